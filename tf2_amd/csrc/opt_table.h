// opt_table.h -- every option of TF2_AMD_OPTS (opts.h), declared ONCE: one line per option, its doc in the comment behind it.
// Adding an option is one line here (and its name in INTEGRATION.md section 5, which tests/test_host_abi.py holds against this file).
//
//   TF2_OPT(name, scope, test_only, type, member, default)     loaded into RunOpts::member (tf2_net.h) by Net::load_options
//   TF2_OPT_RAW(name, scope, test_only, default)               no member of its own: read with opt(OPT_name), or by one of the special
//                                                              rules written out in Net::load_options (net.hip)
//
// scope = when the value is read: pack (tf2_net_pack), create (tf2_net_create), plan (when a launch plan is built: fixed in the plan),
// run (every tf2_net_run), tools (-DTF2_PROBES builds and the timeline tools).  test_only = 1: refused unless TF2_AMD_TEST=1 (forced
// kernels, disabled proofs, thresholds -- the test-suite's and the A/B tools').  The file has no include guard: it is included once per
// use (the OptId enum in opts.h, the parser's table in opts.cpp, the RunOpts members in tf2_net.h, the loop of Net::load_options), each
// with its own definition of the two macros, and undefines them at its end.  Bit masks of rows: bit l = table row l.

// ---- product options (INTEGRATION.md section 5 has them as a table) ----
TF2_OPT(alt_conc, run, 0, int, alt_conc_mode, 2)   // how Net::run decides that batches are in flight: 0 never, 1 always, 2 (default) the caller's tf2_net_run_ex statement, else calls on >= 2 streams among the last eight
TF2_OPT(bgroup, plan, 0, int, bgroup_mode, 1)      // group launches (conv_bgroup.hip: identity bottlenecks of the 28 x 28 / 14 x 14 / 7 x 7 maps in one launch, eight co-resident blocks per image that meet inside the kernel), one batch at a time only: 1 (default) / 0
TF2_OPT(bfirst, plan, 0, int, bfirst_mode, 2)      // the first bottleneck of the 56 x 56 stage (shortcut | reduce, 3x3, expand + residual) as one launch of independent row bands (conv_bfirst.hip): 0 never, 1 with batches in flight, 2 (default) one batch at a time as well (instead of the group launch)
TF2_OPT(bband, plan, 0, int, bband_mode, 1)        // identity bottlenecks as band launches (conv_bband.hip): 0 never, 1 (default) with batches in flight, 2 one batch at a time as well (instead of the group launches: forces bband_alone_maps = 6)
TF2_OPT(c3, plan, 0, int, c3_mode, 1)              // 3x3 / 1 / pad 1 layers of big maps on conv_c3.hip (halo tile in LDS): 1 (default), 0 the ring kernel; 2 / 3 force 64- / 128-channel blocks (tests)
TF2_OPT(img, plan, 0, int, img_mode, 1)            // stride-1 rows of small square maps (ResNet-50's 7 x 7 x 512 3x3 rows) on conv_img.hip (whole images per block, the input resident in LDS) instead of the split-K kernel: 0 never, 1 (default) with batches in flight, 2 one batch at a time as well (the group launches keep their rows)
TF2_OPT(fc, plan, 0, int, fc_mode, 1)              // whole-window layers at batch <= 32 on conv_fc.hip (weight stream): 1 (default) / 0
TF2_OPT_RAW(fc4, pack, 0, 1)                       // conv_fc layers keep their filters as 4-bit codes in HBM (expanded in registers): 1 (default) / 0 int8 window tiles
TF2_OPT_RAW(share, pack, 0, 1)                     // alternative tile heights share the main entry's weight tiles: 1 (default: the wide ones), 2 all, 0 none

// ---- test-only: pack and create time ----
TF2_OPT_RAW(merge, pack, 1, 1)                     // 0 = no merged rows (a 1x1 row and the 3x3 row behind it as one 3x3 layer)
TF2_OPT_RAW(nodbl, pack, 1, 0)                     // no doubled channels
TF2_OPT_RAW(nofuse, pack, 1, 0)                    // no conv_bneck pairs
TF2_OPT_RAW(nodual, pack, 1, 0)                    // two-window layers in the Horner form
TF2_OPT_RAW(nofast, pack, 1, 0)                    // generic requantisation everywhere
TF2_OPT_RAW(nosemi, pack, 1, 0)                    // no SEMI requantisation
TF2_OPT_RAW(nounit, pack, 1, 0)                    // conv1's low window as a window
TF2_OPT_RAW(no4bit, pack, 1, 0)                    // shift-kernel layers keep int32 weights
TF2_OPT_RAW(im2col0, create, 1, 1)                 // 0: a 3x3 first layer on 3 channels keeps its plain form (Net::init; read per handle: tests build both forms)

// ---- test-only: kernel selection and thresholds of the launch plan ----
TF2_OPT(pw, plan, 1, int, pw_mode, 1)              // conv_pw (register-resident pointwise kernel): 1 auto (default), 0 never
TF2_OPT(pw_slabs, plan, 1, int, pw_slabs, 1)       // conv_pw: most K slabs
TF2_OPT(pw_minpix, plan, 1, long, pw_minpix, 8192) // conv_pw: fewest pixels
TF2_OPT(sk, plan, 1, int, sk_mode, 0)              // in-block split-K kernel: 0 auto, 1 forced for every 64-row layer, 2 never
TF2_OPT(sk8, plan, 1, long, sk8_blocks, 128)       // largest split-K grid that takes the 8-wave form
TF2_OPT(sk_s3, plan, 1, long, sk_s3_blocks, 256)   // largest split-K grid on three ring stages (100 KiB of LDS: the block owns its CU), one batch at a time
TF2_OPT(sk_s3_conc, plan, 1, long, sk_s3_blocks_conc, 0)   // ... with batches in flight
TF2_OPT(sk_kb, plan, 1, int, sk_kb, 1)             // split-K launches of at most sk_kb_blocks blocks (batch 1-4: the 7 x 7 and 14 x 14 maps) split K over blocks as well: 1 (default) / 0
TF2_OPT(sk_kb_blocks, plan, 1, int, sk_kb_blocks, 8)   // ... largest grid (64 x 64 output tiles) that takes it (the 7 x 7 maps at batch 1: -3 us per 3x3 row; 16-block grids -- the 14 x 14 maps -- measured 0.3-1.4 us SLOWER: the exchange costs ~3 us)
TF2_OPT(sk_kb_max, plan, 1, int, sk_kb_max, 8)     // ... most blocks per output tile
TF2_OPT(sk_kb_min, plan, 1, int, sk_kb_min, 8)     // ... fewest: the slab list must be long enough for that many parts of eight wave items (two parts of a short list cost GoogLeNet's batch-1 step 25 us)
TF2_OPT(stem, plan, 1, int, stem_mode, 1)          // conv_stem.hip for the executed first layer: 1 auto (default), 0 never
TF2_OPT(stem_pool, plan, 1, int, stem_pool, 1)     // conv1's 3x3 / 2 max pool inside the conv_stem launch: 1 (default) / 0 its own launch
TF2_OPT(stem_pk_small, plan, 1, int, stem_pk_small, 1)   // conv_stem_pool_kernel at small batches with fewer pooled rows per block (a grid of >= ~192 blocks): 1 (default) / 0
TF2_OPT(q128, plan, 1, int, q128_flags, 1)         // the input preparation tells conv_stem_pool_kernel per image whether a -128 is there (no scan of its input tile) where the step starts prep | stem + pool | conv_bfirst: 1 (default) / 0
TF2_OPT(pwk, plan, 1, int, pwk_mode, 1)            // short-K pointwise rows (1x1 rows of 128 / 256 / 512 input channels) on conv_pwk.hip (a block's weight fragments resident in registers, pixel tiles with their whole K extent streamed through LDS) instead of the ring kernel: 0 never, 1 (default) with batches in flight, 2 one batch at a time as well
TF2_OPT(pwk_minpix, plan, 1, long, pwk_minpix, 4096)   // conv_pwk: fewest output pixels
TF2_OPT(pwk_units, plan, 1, int, pwk_min_units, 512)   // conv_pwk: fewest (tile, channel part) units of a row (default 512: two tiles per block and more)
TF2_OPT(pwk_slabs, plan, 1, int, pwk_max_slabs, 4) // conv_pwk: most K slabs of a row (2, 4 or 8; 8 = the 512-channel rows too: 256 registers, no overlapped epilogue -- 1.3 % slower in flight than the ring kernel's pair)
TF2_OPT(pwk_sk, plan, 1, int, pwk_sk, 0)           // conv_pwk: 1 = rows that would take the in-block split-K kernel as well
TF2_OPT(pwk_rows, plan, 1, unsigned long long, pwk_rows, 0)       // bit mask of rows forced onto conv_pwk whatever pwk_units / pwk_minpix / pwk_slabs say, where the kernel can run them at all
TF2_OPT(nopwk_rows, plan, 1, unsigned long long, nopwk_rows, 0)   // ... kept off it
TF2_OPT(pwk_pipe, plan, 1, int, pwk_pipe, 1)       // conv_pwk: 0 = no requantisation between the next column group's MFMAs (the plain epilogue for every row)
TF2_OPT(pwk_slots, plan, 1, int, pwk_slots, 256)   // conv_pwk: blocks a launch aims at (<= 0: 256 too; one per CU: 3-5 tiles per block amortise a block's first-operand wait; 512 measured 0.7 % slower in flight)
TF2_OPT(img_min, plan, 1, int, img_min, 8)         // conv_img: smallest batch that takes it (batch-1 plans keep their K-over-blocks launches)
TF2_OPT(img_rows, plan, 1, unsigned long long, img_rows, 0)       // bit mask of rows taken by conv_img whatever img / img_min say, where the kernel can run them at all
TF2_OPT(noimg_rows, plan, 1, unsigned long long, noimg_rows, 0)   // ... kept off it
TF2_OPT(fc_min, plan, 1, int, fc_min_slabs, 64)    // conv_fc: shortest K (64-byte slabs) that takes it; the packer reads it too (fc4: a layer packed as 4-bit codes can run nowhere else)
TF2_OPT(c3_min, plan, 1, long, c3_min_blocks, 96)  // conv_c3: smallest grid that takes it
TF2_OPT(c3_min_hw, plan, 1, int, c3_min_hw, 14)    // conv_c3: smallest map side
TF2_OPT(c3_min256, plan, 1, long, c3_min256, 200)  // conv_c3: smallest grid of 256-channel blocks (one-window layers; else 128-channel blocks)
TF2_OPT(c3_pool, plan, 1, int, c3_pool, 1)         // a layer's 2x2 / 2 max pool inside its conv_c3 launch (tiles of TH x 32 pixels): 1 (default) / 0 its own launch
TF2_OPT(c3_w9, plan, 1, int, c3_w9, 1)             // conv_c3_w9_kernel: 0 never, 1 (default) where a block walks at least eight tiles, 2 wherever the layer allows it (tests)
TF2_OPT(fire, plan, 1, int, fire_mode, 2)          // a fire module (squeeze + merged expands) as ONE launch (conv_fire.hip): 0 never, 1 wherever it fits, 2 (default) on maps >= 28 wide (14 x 14 modules measured SLOWER fused: 64-128 blocks of long dependent chains, r05_experiments.txt item 10)
TF2_OPT(fire_pool, plan, 1, int, fire_pool, 3)     // fire modules with a pool behind their expands: 0 never, 1 on maps >= 56 wide (the pool stays a launch), 2 wherever `fire` allows (pool a launch), 3 (default) the pool inside the fire launch where its form fits one batch at a time / as 2 with batches in flight, 4 inside always
TF2_OPT(first, plan, 1, int, first_fuse, 1)        // a 3x3 / stride 1 first layer on the 3-channel image as ONE launch with its input preparation (conv_first_kernel): 1 (default) / 0
TF2_OPT(first_pool, plan, 1, int, first_pool, 1)   // ... a 3x3 first layer (stride 1 / 2) with a 3x3 / 2 max pool behind its ReLU, the pool in that launch too (conv_first_pool_kernel): 1 (default) / 0
TF2_OPT(bneck_min, plan, 1, long, bneck_min_blocks, 200)   // conv_bneck: smallest grid that takes it
TF2_OPT(avg_fuse, plan, 1, int, avg_fuse, 2)       // the global average of an end-pool layer inside its split-K launch (conv_mfma_sk AVG): 0 never (global_avg_kernel), 1 always, 2 (default) one batch at a time only
TF2_OPT(pair, plan, 1, int, pair_mode, 1)          // two independent neighbouring rows (shortcut | first 1x1) in one launch: 1 (default) / 0 never; tensor lifetimes depend on it
TF2_OPT(bgroup_min7, plan, 1, int, bgroup_min7, 12)       // smallest batch that takes the group launches of the 7 x 7 maps (a group is 8 CUs per image whatever the batch)
TF2_OPT(bgroup_min14, plan, 1, int, bgroup_min14, 12)     // ... 14 x 14
TF2_OPT(bgroup_min28, plan, 1, int, bgroup_min28, 12)     // ... 28 x 28
TF2_OPT(bgroup_min56f, plan, 1, int, bgroup_min56f, 12)   // ... the first 56 x 56 bottleneck (conv_bgroup56f_kernel)
TF2_OPT(bgroup_chain, plan, 1, int, bgroup_chain, 5)      // consecutive identity bottlenecks of the 28 x 28 / 14 x 14 / 7 x 7 maps per group launch (1: one launch each)
TF2_OPT(bgroup_polls, plan, 1, long, bg_poll_limit, 1 << 24)   // group launches: polls of a meeting before it is reported as failed
TF2_OPT(bgroup_withhold, plan, 1, long, bg_withhold, 0)   // group launches: 1 + index of a block that leaves its group at kernel entry (the failure path of tf2_net_poll_error)
TF2_OPT(bfirst_min, plan, 1, int, bfirst_min, 12)  // conv_bfirst: smallest batch that takes it (14 blocks per image)
TF2_OPT(bband_rows, plan, 1, int, bband_rows, 7)   // band launches: output rows per block with batches in flight
TF2_OPT(bband_rows_alone, plan, 1, int, bband_rows_alone, 2)   // ... one batch at a time
TF2_OPT(bband_rows_dd, plan, 1, int, bband_rows_dd, 7)    // band launches: most rows per block of a 28 x 28 bottleneck whose reduce AND 3x3 are two-window layers (rounds 4-5: 4)
TF2_OPT(bband_min, plan, 1, int, bband_min, 8)     // band launches: smallest batch that takes them
TF2_OPT(bband_alone_maps, plan, 1, int, bband_alone_maps, 0)   // maps that take band launches one batch at a time too, instead of the group launches (bit 1: 28 x 28, bit 2: 14 x 14; bband=2 = both)
TF2_OPT(dense, plan, 1, int, dense_mode, 1)        // gather words of dense layers computed from the step index: 1 (default), 0 = always read from the header tables
TF2_OPT(dense_max, plan, 1, int, dense_max_slabs, 17)     // layers with more K slabs than this on grids of more than one round keep the header tables
TF2_OPT(alt_min, plan, 1, long, alt_min_blocks, 200)      // smallest 128 x 128 grid that takes a layer's wide-tile alternative, one batch at a time; given, it moves alt_min_conc's default with it
TF2_OPT(alt_min_conc, plan, 1, long, alt_min_blocks_conc, 90)   // ... when the caller keeps several batches in flight
TF2_OPT(alt_narrow, plan, 1, long, alt_narrow_blocks, 64) // a 128-row layer takes its 64-row alternative below this many 128 x 128 blocks
TF2_OPT(alt_rows, plan, 1, unsigned long long, alt_rows, 0)       // bit mask of rows forced onto their alternative tile height
TF2_OPT(noalt_rows, plan, 1, unsigned long long, noalt_rows, 0)   // ... kept off it
TF2_OPT(sk_rows, plan, 1, unsigned long long, sk_rows, 0)         // bit mask of 64-row-tile rows forced onto the in-block split-K kernel
TF2_OPT(nosk_rows, plan, 1, unsigned long long, nosk_rows, 0)     // ... kept off it

// ---- test-only: tools ----
TF2_OPT_RAW(exp, tools, 1, 0)                      // timing-probe bits of the -DTF2_PROBES build (tf2_device.h kProbe*, tools/probe_run.py), masked into RunOpts::flags; nothing in the product reads them
TF2_OPT_RAW(skip_layers, tools, 1, -1)             // lo-hi (held as lo << 32 | hi): launches of a layer range left out by Net::run (-DTF2_PROBES builds: results are then wrong, only durations are read)
TF2_OPT_RAW(dbgptr, tools, 1, 0)                   // device buffer for per-layer stamps (RunOpts::dbg)
TF2_OPT_RAW(dbgptr2, tools, 1, 0)                  // device buffer for per-block stamps (RunOpts::dbg2)
TF2_OPT(dbglayer, tools, 1, int, dbg_layer, -1)    // the layer dbgptr2 records

#undef TF2_OPT
#undef TF2_OPT_RAW
