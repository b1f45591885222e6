// sg_opts.h -- the context's range-checked options (sg_ctx_set_option), one
// row each: name, default and bounds.  No HIP here (tests/cpp/opts_test.cc).
#pragma once

#include <cstdint>

// Each regime selects its own path, and an option only forces one, for a test
// or a measurement.  -1 = the regime's choice.  No option is read from the
// environment on a call; sg_ctx_create seeds the diagnostics ones (debug_part,
// bucket_blocks, prefix_pairs, flag_skip) from SG_DEBUG_PART /
// SG_BUCKET_BLOCKS / SG_PREFIX_PAIRS / SG_FLAG_SKIP for the GPU scripts.
// (max_launch_records, owner_key_space, debug_part and flag_skip_u16 are no rows here: sg_ctx.hip)
enum SgOpt : int {
  kOptBucketBlocks = 0, kOptPrefixPairs, kOptFoldMap, kOptMinimizeFilter, kOptMinimizeFilterRanks, kOptReportDirect,
  kOptRpcEncodeElems, kOptRpcDecodeBlocks, kOptHostSlice, kOptHostCopyThreads, kOptM0Filter, kOptM0Halves,
  kOptExecCompsPath, kOptFlagSkip, kOptFlagSkipSplit, kOptExecCoverPath,
  kOptCount
};

struct SgOptRow {
  const char* name;
  int64_t def, lo, hi;
};

// in SgOpt's order
constexpr SgOptRow kSgOpts[] = {
    {"bucket_blocks", 0, 0, 1 << 20},         // cap of the persistent bucket grid (0: none)
    {"prefix_pairs", 0, 0, 1},                // prefix_begin's form when the caller passes -1 (0 kept, 1 pairs)
    {"fold_map", -1, -1, 1},                  // one-group fold: -1 by range, 0 never the byte map
    {"minimize_filter", 1, 0, 1},             // Minimize's value filter: 1 on, 0 off
    {"minimize_filter_ranks", 0, 0, 1 << 20}, // Minimize phase A length (0: the default)
    {"report_direct", 0, 0, 1},               // cover report: 1 the global-search form at any size
    {"rpc_encode_elems", -1, -1, 1},          // delta encode: -1 by shape, 0 per-list, 1 per-element
    {"rpc_decode_blocks", -1, -1, 1},         // delta decode: -1 by shape, 0 per-list, 1 per-block
    {"host_slice", 0, 0, 1ll << 40},          // host ingest: entries per record slice (0: the default)
    {"host_copy_threads", 0, 0, 64},          // host ingest: pageable -> pinned copy threads (0: from the CPU quota)
    {"m0_filter", -1, -1, 1},  // the flags path's M0 filter (sg_m0filter.hip): -1 by the last batches, 0 never, 1 tried
    {"m0_filter_halves", -1, -1, 2},  // the filter's index per slice in 2^k parts (-1 by its fill, 0..2 forced)
    {"exec_comps_path", -1, -1, 0},   // sg_exec_comps: -1 by each call's distinct records, 0 always the general path
    // bucket stage in two launches, the second skipping the flag stores of fully queued record blocks
    // (sg_bucket.hip): -1 by the last partitioned slice, 0 never, 1 always
    {"flag_skip", -1, -1, 1},
    {"flag_skip_split", 3, 1, 8},  // ... the first launch takes the first 1 / 2^k of the bucket list
    {"exec_cover_path", -1, -1, 0},  // sg_exec_cover: -1 by each call's distinct PCs, 0 always the general path
};
static_assert(sizeof(kSgOpts) / sizeof(kSgOpts[0]) == kOptCount, "one row per SgOpt");
