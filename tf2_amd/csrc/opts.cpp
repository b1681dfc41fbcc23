// opts.cpp -- the parser behind TF2_AMD_OPTS (opts.h) and its snapshot; the options themselves are opt_table.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <unistd.h>
#include <memory>
#include <mutex>
#include "opts.h"

extern char** environ;

namespace tf2 {

namespace {
struct OptSpec { const char* name; int test_only; long long dflt; };
const OptSpec kOptSpecs[OPT_COUNT] = {                    // indexed by OptId
#define TF2_OPT(name, scope, test_only, type, member, dflt) {#name, test_only, dflt},
#define TF2_OPT_RAW(name, scope, test_only, dflt) {#name, test_only, dflt},
#include "opt_table.h"
};

struct Snapshot {
  long long value[OPT_COUNT]; bool given[OPT_COUNT] = {};
  Snapshot() { for (int i = 0; i < OPT_COUNT; i++) value[i] = kOptSpecs[i].dflt; }
};
std::mutex g_mu;
std::shared_ptr<const Snapshot> g_snap = std::make_shared<Snapshot>();

int find_spec(const std::string& n) {                     // OptId, OPT_COUNT = no such option
  int i = 0;
  while (i < OPT_COUNT && n != kOptSpecs[i].name) i++;
  return i;
}
}  // namespace

long long opt(OptId id) { return std::atomic_load(&g_snap)->value[id]; }
bool opt_given(OptId id) { return std::atomic_load(&g_snap)->given[id]; }

std::string opts_reload() {
  std::lock_guard<std::mutex> lock(g_mu);
  auto snap = std::make_shared<Snapshot>();
  const char* env = getenv("TF2_AMD_OPTS");
  const char* test = getenv("TF2_AMD_TEST");
  const bool test_mode = test && atoi(test) != 0;
  std::string err;
  if (env) {
    std::string text(env);
    size_t pos = 0;
    while (pos <= text.size()) {
      size_t end = text.find_first_of(",; ", pos);
      if (end == std::string::npos) end = text.size();
      std::string item = text.substr(pos, end - pos);
      pos = end + 1;
      if (item.empty()) continue;
      std::string name = item, val = "1";
      const size_t eq = item.find('=');
      if (eq != std::string::npos) { name = item.substr(0, eq); val = item.substr(eq + 1); }
      if (eq != std::string::npos && val.empty()) { err = "TF2_AMD_OPTS: '" + item + "' has no value (a bare name means name=1)"; break; }
      const int id = find_spec(name);
      if (id == OPT_COUNT) { err = "TF2_AMD_OPTS: unknown option '" + name + "'"; break; }
      if (kOptSpecs[id].test_only && !test_mode) { err = "TF2_AMD_OPTS: '" + name + "' is a test-only option (set TF2_AMD_TEST=1 as well)"; break; }
      long long v;
      if (id == OPT_skip_layers) {                        // lo-hi -> lo << 32 | hi
        int lo = 0, hi = -1;
        if (sscanf(val.c_str(), "%d-%d", &lo, &hi) != 2) { err = "TF2_AMD_OPTS: skip_layers wants lo-hi"; break; }
        v = ((long long)lo << 32) | (unsigned)hi;
      } else {
        char* endp = nullptr;
        v = (long long)strtoull(val.c_str(), &endp, 0);
        if (val[0] == '-') v = strtoll(val.c_str(), &endp, 0);
        if (!endp || *endp) { err = "TF2_AMD_OPTS: '" + item + "' is not name=integer"; break; }
      }
      snap->value[id] = v; snap->given[id] = true;
    }
  }
  // Rounds 1-4 read 56 separate TF2_AMD_* variables (TF2_AMD_BGROUP=0, TF2_AMD_ALT_CONC, ...).  A deployment that still sets one of
  // them -- e.g. to keep the group launches off where their preconditions cannot be guaranteed -- must not silently get the default
  // back: any TF2_AMD_* name other than the four the library reads is an error that names its replacement.
  if (err.empty()) {
    static const char* const kKnown[] = {"TF2_AMD_OPTS", "TF2_AMD_TEST", "TF2_AMD_LIB", "TF2_AMD_TOOL_LIB"};
    for (char** e = environ; e && *e; e++) {
      if (strncmp(*e, "TF2_AMD_", 8) != 0) continue;
      const char* eqp = strchr(*e, '=');
      const std::string nm(*e, eqp ? (size_t)(eqp - *e) : strlen(*e));
      bool known = false;
      for (const char* k : kKnown) known = known || nm == k;
      if (known) continue;
      std::string low = nm.substr(8);
      for (char& c : low) c = (char)tolower((unsigned char)c);
      err = "environment variable " + nm + " is no longer read: use TF2_AMD_OPTS=\"" + low + "=" + (eqp ? eqp + 1 : "1") + "\"" +
            (find_spec(low) != OPT_COUNT ? "" : " (INTEGRATION.md section 5 lists the current names)");
      break;
    }
  }
  if (!err.empty()) return err;                           // (the previous snapshot stays)
  std::atomic_store(&g_snap, std::shared_ptr<const Snapshot>(snap));
  return std::string();
}

}  // namespace tf2
