// opts.h -- TF2_AMD_OPTS: the ONE run-time option string of the library (round 5; rounds 1-4 had grown 56 separate TF2_AMD_*
// environment variables, read with getenv() in packers, planners and launchers).
//
//   TF2_AMD_OPTS="name=value,name=value,flag"        (a bare name means name=1)
//
// Parsed ONCE per tf2_net_create / tf2_net_reload_options into an immutable snapshot that every later read takes from (no getenv()
// anywhere else: launchers run on several feeder threads, and getenv racing with a setenv is undefined behaviour).  Unknown names are
// an error (TF2_ERR_ARG from create / reload), and so is a TEST-ONLY option unless TF2_AMD_TEST=1 is set as well: those force
// kernels, disable proofs or lower thresholds for the test-suite and the A/B tools and are no part of the product's interface.
// Every option -- name, default, doc -- is one line of opt_table.h; INTEGRATION.md section 5 documents the product options.
#pragma once
#include <string>

namespace tf2 {

enum OptId {                                          // OPT_<name> for every line of opt_table.h: a misspelt name does not compile
#define TF2_OPT(name, scope, test_only, type, member, dflt) OPT_##name,
#define TF2_OPT_RAW(name, scope, test_only, dflt) OPT_##name,
#include "opt_table.h"
  OPT_COUNT
};

long long opt(OptId id);                              // value of the option in the current snapshot: the table's default when it is not set
bool opt_given(OptId id);                             // the option string sets it
std::string opts_reload();                            // re-read TF2_AMD_OPTS / TF2_AMD_TEST; error text, empty = ok

}  // namespace tf2
