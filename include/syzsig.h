/*
 * syzsig.h -- C-ABI of the MI355X coverage-signal triage engine (libsyzsig.so).
 *
 * This is the drop-in boundary for syzkaller's coverage-signal path.  Every
 * entry point names the reference interface it replaces (paths relative to the
 * syzkaller checkout).  The Go side binds it through cgo; INTEGRATION.md shows
 * the binding.  Plain pointers and sizes only.
 *
 * Conventions
 *  - Every function returning int returns SG_OK (0) or a negative SG_E* code;
 *    sg_last_error() gives the message (thread-local).  The Go adapter panics
 *    on failure, as the reference callers do (syz-fuzzer/fuzzer.go:389-391).
 *  - "host" entry points take caller-owned host memory and never retain it
 *    (cgo pointer rules).  "_dev" entry points take device pointers already
 *    resident in HBM and are stream-ordered on the context's stream: they do
 *    not synchronise, and their outputs are valid after sg_ctx_sync().
 *  - Signal / cover values are uint32_t, any value allowed.  Sorted-slice ops
 *    follow pkg/cover/cover.go exactly: multiset semantics; 0xFFFFFFFF
 *    (`sent`, cover.go:17) is dropped by every foreach op (cover.go:97), and
 *    by Canonicalize only when no smaller value precedes it (`last` starts at
 *    sent, cover.go:31).
 *  - A context owns one HIP stream on one device and all device memory it
 *    allocates.  Calls on one context must be serialised by the caller (the
 *    reference already holds signalMu / mgr.mu around them).
 *  - There is no CPU fallback: without a usable gfx950 device every call that
 *    computes returns SG_ENODEV.
 */
#ifndef SYZSIG_H
#define SYZSIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK 0
#define SG_EINVAL (-1)
#define SG_EHIP (-2)
#define SG_ENOMEM (-3)
#define SG_ENODEV (-4)

typedef struct sg_ctx sg_ctx;
typedef struct sg_set sg_set;

/* Library identification and error reporting. */
const char* sg_version(void);
const char* sg_last_error(void);

/* ---- context ------------------------------------------------------------ */
/* One per fuzzer / manager process (or per GPU rank).  `device` is the HIP
 * device ordinal. */
int sg_ctx_create(int device, sg_ctx** out);
void sg_ctx_destroy(sg_ctx* ctx);
/* Wait for all work queued on the context's stream. */
int sg_ctx_sync(sg_ctx* ctx);
/* Queue all further work on `hip_stream` (e.g. torch's current stream; NULL is
 * the legacy default stream).  The context's own stream is a blocking stream,
 * i.e. ordered with the legacy default stream. */
int sg_ctx_set_stream(sg_ctx* ctx, void* hip_stream);
/* Go back to the context's own stream. */
int sg_ctx_reset_stream(sg_ctx* ctx);
void* sg_ctx_stream(sg_ctx* ctx);
/* Per-kernel device timing with HIP events on the context's stream.
 * enable != 0 starts recording (and resets the tallies). */
int sg_ctx_timing(sg_ctx* ctx, int enable);
/* Total device milliseconds and launch count recorded for kernel `name`
 * (e.g. "bucket_triage"); syncs the stream. */
int sg_ctx_kernel_time(sg_ctx* ctx, const char* name, double* ms, uint64_t* launches);
/* Context counters: "owner_resets" (Minimize's first-owner table generations
 * started after the key space ran out), "owner_floor", "owner_key_space",
 * "max_launch_records"; the host ingest's last call (sg_triage_batch /
 * sg_triage_traces without diff lists): "host_copy_bytes", "host_copy_ns"
 * (pageable -> pinned copies), "host_wait_ns" (waits for a staging slot's DMA),
 * "host_copy_threads"; "cpu_quota_milli" (the CPUs this process may use,
 * x1000); "workspace_bytes" (the capacity of the context's grow-only device
 * workspace: 0 before the first call that needs it, then 64 MiB, doubling);
 * the M0 filter (the flags path's low-novelty regime): "m0_filter_used"
 * and "m0_filter_fallback" (record slices it finished / that went on to pass
 * 2), "m0_filter_survivors" (the last launch's), "m0_filter_queued_milli" (the
 * queued fraction of the last partitioned slice, x1000, that auto reads),
 * "m0_filter_halves_log" (the index parts per slice, log2, auto uses now);
 * "flag_skip_used" (bucket launches run in two phases), "flag_skip_full_blocks"
 * (fully queued 4096-record blocks the last of them found after its first phase),
 * "flag_skip_all_flagged" (those that found every block so and ran their second
 * phase without the owner map), "flag_skip_u16" (those whose pass 2 over the
 * slices after the first window ran late, in 2-byte entries);
 * "hints_candidates" (the last sg_hints_replacers* call's (slot, pair)
 * matches, before deduplication); "exec_comps_general" (the calls the last
 * sg_exec_comps* call sent down its general path), "exec_comps_fast_cap"
 * (SG_EXEC_COMPS_FAST_CAP), and the same two of sg_exec_cover*,
 * "exec_cover_general" and "exec_cover_fast_cap"; "triage_runs_wide" (the
 * candidates of the last sg_triage_runs_from_kcov* call that held a cover list
 * not non-decreasing as u32; counted on the device, read here after a stream
 * sync), and of the same call the candidates whose inputCover took each route
 * of the fold, counted and read the same way: "triage_runs_copied" (one list:
 * a copy), "triage_runs_sorted" (two or more ascending lists of at most
 * "triage_runs_sort_cap" values together: sorted in LDS), "triage_runs_ranked"
 * (more values than that: by ranks), "triage_runs_foreach" (a wide list, one
 * that starts with the sentinel, or offsets that give the lists more values
 * than the candidate's PCs: the two-pointer loop itself); candidates with another
 * status than SG_TIN_OK or without a cover list are in none of the four;
 * "triage_runs_sort_cap" and "tinput_chunk" (constants: the values of new_k
 * that sg_triage_intersect / sg_triage_subset and the run loop of
 * sg_triage_runs_from_kcov* hold in LDS at a time); "prio_bad_ids" (the call
 * ids >= ncalls that sg_prio_table_add_dev has skipped on this context since
 * it was created; counted on the device, read here after a stream sync),
 * "prio_band_cells" and "prio_short_len" (constants: the u32 cells of a row
 * band that the pair count keeps in LDS, and the longest program that takes
 * the band path); "sha1_long_progs" (the programs that took the long SHA-1
 * path of sg_prog_hashes*, sg_sigset_add_progs and sg_hub_sync on this
 * context since it was created; counted on the device, read here after a
 * stream sync) and "sha1_long_len" (constant: SG_SHA1_LONG);
 * "inflate_long_streams" (the streams that took the wave-per-stream path of
 * sg_inflate_batch*, sg_db_open on this context since it was created, once
 * per call that counted them; counted on the device, read here after a stream
 * sync) and "inflate_long_len" (constant: SG_INFLATE_LONG);
 * "deflate_long_streams" (likewise for sg_deflate_batch*, sg_db_serialize and
 * sg_db_compact) and "deflate_long_len" (constant: SG_DEFLATE_LONG);
 * "deflate_stored_streams", "deflate_fixed_streams" and
 * "deflate_dynamic_streams" (the streams of the last such call per form,
 * summing to its streams; a database call counts a deletion or an empty value
 * as the two-byte fixed stream it does not write);
 * "owned_big_records" (the
 * records the last
 * ordered-output call -- sg_triage_batch[_dev] with diff lists, sg_merge_poll
 * -- swept a workgroup each instead of a wave each, summed over its record
 * slices; counted on the device and read here after a stream sync, so the
 * call itself gains no wait); the paths of the last merge (sg_merge,
 * sg_merge_batch, and the merges inside sg_union_fold), in pairs, summing to
 * the batch: "merge_pairs_generic" (keep masks, scan and scatter: the whole
 * batch as soon as one pair has no side of <= 4096 values -- for Difference /
 * Intersection, a first list above 4096 -- or holds 2^32 values or more),
 * "merge_pairs_diff_small" (Difference / Intersection, a workgroup per pair),
 * "merge_pairs_gap" and "merge_pairs_tile" (Union / SymmetricDifference, a
 * workgroup per pair: the large side at least 32x the small one, and the
 * rest); the paths of the last Canonicalize (sg_canonicalize[_batch], and the
 * one inside sg_triage_newsig): "canon_wave_lists" and "canon_block_lists"
 * (non-empty lists of <= 1024 and of 1025..4096 values when no list is
 * longer: sort and unique in one pass), "canon_big_segments" (lists above
 * 4096; non-zero: the whole batch took the tile sort, the rank-merge passes
 * and the separate unique pass, and the two list counts are 0),
 * "canon_merge_passes" (its rank-merge launches).  These eight are host
 * arithmetic over the call's lengths; a call that ends before any device work
 * (no pairs, two empty lists, no values) leaves them unchanged. */
int sg_ctx_counter(sg_ctx* ctx, const char* name, uint64_t* out);
/* Context options.  Every path is selected by its regime; an option only
 * forces one, for a test or a measurement, and no call reads the environment
 * (sg_ctx_create seeds "debug_part", "bucket_blocks", "prefix_pairs" and
 * "flag_skip" from SG_DEBUG_PART / SG_BUCKET_BLOCKS / SG_PREFIX_PAIRS /
 * SG_FLAG_SKIP, and "flag_skip_u16" from SG_FLAG_SKIP_U16, for the GPU scripts).
 * Keys (-1 = the regime's choice where it applies):
 *   "max_launch_records"   records per partitioned launch (0: 2^24)
 *   "owner_key_space"      Minimize's first-owner key space (0: 2^32 - 1; set
 *                          before the first Minimize)
 *   "debug_part"           phase counters of the partitioned path (stderr)
 *   "bucket_blocks"        cap of the persistent bucket grid (0: none)
 *   "prefix_pairs"         sg_prefix_begin_dev's form (0 kept partitions, 1 pairs)
 *   "fold_map"             sg_union_fold's one-group byte map (-1 by range, 0 never)
 *   "minimize_filter"      Minimize's value filter (1 on, 0 off)
 *   "minimize_filter_ranks" Minimize's phase-A inputs (0: the default 4)
 *   "report_direct"        sg_cover_uncovered's and sg_cover_lines' global-search form at any size (1)
 *   "rpc_encode_elems"     delta encode form (-1 by shape, 0 per list, 1 per element)
 *   "rpc_decode_blocks"    delta decode form (-1 by shape, 0 per list, 1 per block)
 *   "host_slice"           host ingest: entries per record slice (0: 64 Mi)
 *   "host_copy_threads"    host ingest: copy threads (0: half the CPU quota, 2..16)
 *   "m0_filter"            the flags path's M0 filter (-1 auto: after a filtered
 *                          slice, or a partitioned one that queued < 1/4 of its
 *                          records, backing off after fallbacks; 1 always; 0 never)
 *   "m0_filter_halves"     its index in 2^k parts per slice (-1 auto: 2 parts once a
 *                          part overflows; 0..2 forced)
 *   "exec_comps_path"      sg_exec_comps' path (-1 by each call's distinct records,
 *                          0 the general path for every call)
 *   "exec_cover_path"      sg_exec_cover's path (-1 by each call's distinct PCs,
 *                          0 the general path for every call)
 *   "flag_skip"            the flags path's bucket stage in two launches, the second
 *                          skipping the flag stores of record blocks the first left
 *                          fully queued (-1 auto: after a partitioned slice that
 *                          queued most of its records; 1 always; 0 never)
 *   "flag_skip_split"      k, 1..8: the first launch takes 1 / 2^k of the bucket list
 *   "flag_skip_u16"        a split launch of the flags path scatters pass 2 around its
 *                          first launch: the slices of the first window before it, the
 *                          others after the flag summary, in 2-byte entries when every
 *                          record is flagged (-1 whenever the launch splits; 0 never:
 *                          pass 2 whole, before the bucket stage; 1 with the split forced)
 * Unknown keys and out-of-range values return SG_EINVAL. */
int sg_ctx_set_option(sg_ctx* ctx, const char* key, int64_t value);
int sg_ctx_get_option(sg_ctx* ctx, const char* key, int64_t* out);
/* Profiling aid: a one-thread kernel (k_mark_begin, or k_mark_end when end !=
 * 0) on the context's stream, so a kernel trace can cut out a region. */
int sg_ctx_marker(sg_ctx* ctx, int end, uint32_t tag);

/* ---- signal sets: replace map[uint32]struct{} ---------------------------- */
/* maxSignal / corpusSignal / newSignal (syz-fuzzer/fuzzer.go:65-68) and
 * corpusSignal / maxSignal / corpusCover (syz-manager/manager.go:71-73): a
 * direct-indexed 2^32-bit bitmap (512 MiB) resident in HBM. */
int sg_set_create(sg_ctx* ctx, sg_set** out);
void sg_set_destroy(sg_set* set);
int sg_set_clear(sg_set* set);
/* len(map) */
int sg_set_count(sg_set* set, uint64_t* out);
/* All members ascending (the reference iterates map order; payloads of
 * ConnectRes.MaxSignal / PollArgs.MaxSignal, pkg/rpctype/rpctype.go).  Writes
 * min(count, cap) values; *n = count. */
int sg_set_export(sg_set* set, uint32_t* out, size_t cap, size_t* n);
/* pkg/cover/cover.go:178-182  SignalAdd(base, signal) */
int sg_set_add(sg_set* set, const uint32_t* sig, size_t n);
/* pkg/cover/cover.go:160-167  SignalNew(base, signal) -> *out 0/1 */
int sg_set_new(sg_set* set, const uint32_t* sig, size_t n, int* out);
/* pkg/cover/cover.go:169-176  SignalDiff(base, signal): members of sig not in
 * base, in order, duplicates kept.  out capacity n; *nout = count. */
int sg_set_diff(sg_set* set, const uint32_t* sig, size_t n, uint32_t* out, size_t* nout);
/* Device bitmap (2^27 uint32 words) for collectives (OR-reduce across ranks).
 * Layout: signal s = bytes (b3 b2 b1 b0) is bit p = (b2 b1 b3 b0) (bit p & 31
 * of word p >> 5), a fixed permutation of whole words that keeps each (b2, b1)
 * block of 2^16 signals contiguous (the triage's buckets).  Element-wise ops
 * (OR, copy, count) do not depend on it. */
void* sg_set_device_words(sg_set* set);
/* Wrap caller-owned device memory (2^27 uint32 words, e.g. a torch tensor)
 * as a set without copying; sg_set_destroy then frees only the handle. */
int sg_set_wrap_dev(sg_ctx* ctx, void* d_words, sg_set** out);
/* set |= words (device pointer to 2^27 uint32 words). */
int sg_set_or_dev(sg_set* set, const uint32_t* d_words);
/* set |= words & ~exclude (device pointer to 2^27 uint32 words; exclude a set
 * of the same context): the new signal of a batch whose total was computed
 * against an older maxSignal (fuzzer.go:674 adds to newSignal only what
 * maxSignal lacks). */
int sg_set_or_new_dev(sg_set* set, const uint32_t* d_words, sg_set* exclude);
/* Both in one pass over words: newsig |= words & ~maxsig, then maxsig |= words
 * (newsig nullable; the two sets distinct, of one context, neither aliasing
 * words).  Words that are zero are read once and nothing else is touched. */
int sg_set_or_new_or_dev(sg_set* newsig, sg_set* maxsig, const uint32_t* d_words);
/* dst = src (both sets of the same context). */
int sg_set_copy(sg_set* dst, sg_set* src);
/* *out = number of the n device-resident values not in set (duplicates
 * counted), i.e. the candidates a triage of them would test; syncs. */
int sg_set_count_missing_dev(sg_set* set, const uint32_t* d_vals, uint64_t n, uint64_t* out);

/* ---- batched new-signal triage (THE hot path) ----------------------------- */
/* syz-fuzzer/fuzzer.go:645-693 execute(): for call records r = 0..nrec-1 in
 * sequential (program-major, call-index) order, record r's signal is
 * vals[rec_off[r] .. rec_off[r+1]).  Exactly as the sequential loop:
 *   rec_new[r] = SignalNew(maxSignal, S_r) at its turn (fuzzer.go:666);
 *   diff_r     = SignalDiff(maxSignal, S_r) at its turn (fuzzer.go:669);
 *   maxSignal ∪= diff_r; newSignal ∪= diff_r (fuzzer.go:673-674).
 * diff_r is written to diff_vals[diff_off[r] .. diff_off[r+1]) when diff_vals /
 * diff_off are non-NULL (capacity = rec_off[nrec]).  newsig may be NULL.
 * *n_diff (nullable) = total diff elements. */
int sg_triage_batch(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* vals, const uint64_t* rec_off,
		    size_t nrec, uint8_t* rec_new, uint32_t* diff_vals, uint64_t* diff_off, uint64_t* n_diff);
/* Same, device-resident: d_vals (nvals = rec_off[nrec] elements), d_rec_off
 * (nrec+1), outputs d_rec_new (nrec bytes), optional d_diff_vals (capacity
 * nvals), d_diff_off (nrec+1).  Stream-ordered, no host synchronisation,
 * except that a flags-only batch of more than 2^24 records runs as record
 * slices with one small device-to-host read per slice.  Limits: nvals <
 * 2^32 - 2^15, nrec < 2^32 - 1. */
int sg_triage_batch_dev(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* d_vals,
			const uint64_t* d_rec_off, uint64_t nvals, uint64_t nrec, uint8_t* d_rec_new,
			uint32_t* d_diff_vals, uint64_t* d_diff_off);

/* The same triage fed with raw per-call u32 PC traces (the executor's KCOV
 * buffers, executor/executor_linux.cc:262-313) instead of signal: record r =
 * call r, its trace pcs[call_off[r] .. call_off[r+1]) (call_off[0] == 0),
 * its edges sig = pc ^ hash(previous pc of the call), pc ^ 0 for the call's
 * first pc (executor/executor.h:389-401, hash :497-505), zero edges dropped
 * (dedup(0) reports seen, :507-526).  rec_new and the maxSignal / newSignal
 * updates are exactly those of sg_exec_signal_dev followed by a flags-only
 * sg_triage_batch_dev on its output: the executor writes every non-zero edge
 * at its first occurrence in the program, so the first call holding each
 * edge and the batch's union of edges -- all that decides the flags and the
 * sets (fuzzer.go:665-691) -- do not depend on the edges its lossy dedup
 * table drops or lets through again (set-exact mode).
 * Calls need not be grouped into programs.  Limits as sg_triage_batch_dev. */
int sg_triage_traces(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* pcs, const uint64_t* call_off,
		     size_t ncalls, uint8_t* rec_new);
int sg_triage_traces_dev(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* d_pcs,
			 const uint64_t* d_call_off, uint64_t npcs, uint64_t ncalls, uint8_t* d_rec_new);

/* ---- one batch hash-sharded by signal across GPUs ------ */
/* The sequential loop of sg_triage_batch (syz-fuzzer/fuzzer.go:645-693) over a
 * batch whose call records are split contiguously across G ranks, one GPU each
 * (the host protocol and its RCCL exchanges: syzkaller_amd/shard.py).  The
 * signal space is sharded by sg_shard_of(s, G), the murmur3 finaliser of s
 * scaled to [0, G); G <= 64.  Every rank holds the same maxSignal snapshot. */
int sg_shard_of(uint32_t s, uint32_t nshards);
/* Local stage, on the rank holding records rec_base .. rec_base+nrec-1 of the
 * batch (d_rec_off[0] == 0, rec_base + nrec < 2^32): every distinct s of those
 * records that is not in `snapshot`, once, as the pair {s, rec_base + its
 * first record}, grouped by owning shard: shard k's pairs are pairs
 * d_shard_off[k] .. d_shard_off[k+1]-1 of d_pairs (u32 pairs, capacity nvals
 * pairs; d_shard_off: G+1 device u64).  The snapshot is only read.  Any
 * number of entries (record slices of < 2^30 entries each). */
int sg_shard_candidates_dev(sg_ctx* ctx, sg_set* snapshot, const uint32_t* d_vals, const uint64_t* d_rec_off,
			    uint64_t nvals, uint64_t nrec, uint64_t rec_base, uint32_t nshards, uint32_t* d_pairs,
			    uint64_t* d_shard_off);
/* Owner stage, on the shard's rank, over the npairs pairs {s, record} it
 * received from all ranks (record < nrec_total, the batch's record count):
 * owner(s) = the smallest record holding s.  Sets bit r of d_rec_bits (nrec_total
 * bits, cleared first) for every owner record r -- record r is queued for
 * triage iff some shard sets its bit (fuzzer.go:678-690) -- and writes every
 * distinct s once to d_new_vals (capacity npairs); *d_nnew (device u64) = count. */
int sg_shard_owners_dev(sg_ctx* ctx, const uint32_t* d_pairs, uint64_t npairs, uint64_t nrec_total,
			uint32_t* d_rec_bits, uint32_t* d_new_vals, uint64_t* d_nnew);
/* d_rec_new[i] = bit rec_lo + i of the OR of nparts record bitsets, part k
 * being words k*words_per_part .. of d_bits, each starting at word rec_lo/32. */
int sg_shard_flags_dev(sg_ctx* ctx, const uint32_t* d_bits, uint32_t nparts, uint64_t words_per_part, uint64_t rec_lo,
		       uint64_t nrec, uint8_t* d_rec_new);
/* SignalAdd of n device-resident values (fuzzer.go:673-674 for the new signal
 * every shard found). */
int sg_set_add_dev(sg_set* set, const uint32_t* d_vals, uint64_t n);
/* maxsig |= the n device values; newsig (nullable) gains those maxsig lacked
 * before this call (fuzzer.go:673-674: newSignal.Merge(diff), diff =
 * maxSignal.Diff(sig)), duplicates in the values included.  The sparse form of
 * the prefix protocol's set updates (syzkaller_amd/shard.py). */
int sg_set_add_new_dev(sg_set* newsig, sg_set* maxsig, const uint32_t* d_vals, uint64_t n);
/* Clears the bits of the n device values (the sparse prefix protocol clears
 * the prefix bits it set, so the bitmap stays zero between batches). */
int sg_set_del_dev(sg_set* set, const uint32_t* d_vals, uint64_t n);
/* Bitmap prefix exchange of the prefix protocol (syzkaller_amd/shard.py
 * PrefixTriage): d_parts holds nparts bitmap slices of `words` u32 words each,
 * part k from rank k.  d_prefix[k] = OR of parts 0..k-1 (part 0: zero),
 * d_total = OR of all parts.  RCCL has no bitwise-OR reduction. */
int sg_bitmap_prefix_or_dev(sg_ctx* ctx, const uint32_t* d_parts, uint32_t nparts, uint64_t words, uint32_t* d_prefix,
			    uint32_t* d_total);
/* One rank's share of it (the gather form, where every rank holds all parts):
 * d_prefix (nullable: rank 0's is zero) = OR of parts 0..rank-1, d_total = OR
 * of all parts; rank < nparts. */
int sg_bitmap_prefix_or_rank_dev(sg_ctx* ctx, const uint32_t* d_parts, uint32_t nparts, uint64_t words, uint32_t rank,
				 uint32_t* d_prefix, uint32_t* d_total);
/* The two halves of sg_triage_batch_dev (flags and set updates, no diff) for
 * the prefix protocol.  Begin: marks (base != marks) = every signal of the
 * batch not in base (the local new signal, fuzzer.go:666), and
 * each such signal's first record in the batch is kept in the context's slot
 * (0 or 1: two batches can be kept, so one batch's exchange runs while the
 * next is begun).  End: the
 * sequential loop's flags (fuzzer.go:645-693) of the batch's nrec records
 * against maxsig | d_prefix (d_prefix: nullable, 2^27 words in the set layout,
 * e.g. another set's or an exchanged bitmap), written to d_rec_new; maxsig must
 * contain begin's base.  End's set updates: newsig (nullable) gains the new
 * signal (marks minus maxsig | d_prefix), and maxsig |= marks -- its new signal
 * and bits of d_prefix (the prefix protocol ORs a superset of d_prefix into
 * maxsig afterwards).  Flags: the flags without newsig; maxsig ends between
 * its value and maxsig | marks | d_prefix (the protocol ORs a superset of
 * marks | d_prefix into it next), so maxsig is written by flags too.  Marks must stay unchanged until end; only begin's launches read the
 * batch's buffers, and other calls may run on the context between begin and
 * end/flags (the slots have workspaces of their own).  End and flags close
 * the slot. */
int sg_prefix_begin_dev(sg_ctx* ctx, uint32_t slot, sg_set* base, sg_set* marks, const uint32_t* d_vals,
			const uint64_t* d_rec_off, uint64_t nvals, uint64_t nrec);
/* sg_prefix_begin_dev with the batch's form chosen by the caller (there:
 * SG_PREFIX_PAIRS): form 0 keeps the batch's partitions (end re-runs the bucket
 * stage against maxsig | d_prefix), form 1 its distinct signals not in base
 * with their first records (end tests those pairs; cheaper when few).  The
 * results are the same.  d_ncand (nullable, device u64) receives the number of
 * distinct signals of the batch not in base -- the novelty a caller picks the
 * next batch's form from (syzkaller_amd/shard.py PrefixTriage).  Form 2 (base,
 * marks and d_ncand NULL) keeps the partitions and marks nothing: begin + end
 * with d_prefix NULL is sg_triage_batch_dev (flags and set updates) cut in
 * two, so a caller can partition batch i+1 (begin, on one stream) while batch
 * i's bucket stage runs (end, on another; the fuzzer loop's order is kept by
 * running the ends in batch order). */
int sg_prefix_begin_form_dev(sg_ctx* ctx, uint32_t slot, uint32_t form, sg_set* base, sg_set* marks,
			     const uint32_t* d_vals, const uint64_t* d_rec_off, uint64_t nvals, uint64_t nrec,
			     uint64_t* d_ncand);
int sg_prefix_end_dev(sg_ctx* ctx, uint32_t slot, sg_set* maxsig, const uint32_t* d_prefix, sg_set* newsig,
		      uint8_t* d_rec_new);
/* The signals of a pairs-form begin's kept pairs (slot's batch: each
 * distinct signal of the batch not in base, once), d_out[i] for i < min(n,
 * cap), n = the count begin wrote to d_ncand.  The candidate lists the sparse
 * prefix exchange all-gathers (shard.py PrefixTriage) instead of bitmaps;
 * fuzzer.go:665-691 over one batch spread across ranks. */
int sg_prefix_cands_dev(sg_ctx* ctx, uint32_t slot, uint32_t* d_out, uint64_t cap);
int sg_prefix_flags_dev(sg_ctx* ctx, uint32_t slot, sg_set* maxsig, const uint32_t* d_prefix,
			uint8_t* d_rec_new);

/* syz-fuzzer/fuzzer.go:467-489 addInput(), over n inputs in order:
 * diff = SignalDiff(maxSignal, S_k); corpusSignal ∪= diff; maxSignal ∪= diff. */
int sg_add_inputs(sg_ctx* ctx, sg_set* corpus, sg_set* maxsig, const uint32_t* vals, const uint64_t* off, size_t n);

/* syz-fuzzer/fuzzer.go:521-611 triageInput()'s signal math, over n inputs at
 * once (the -procs triage goroutines, or a batch of triage candidates).
 * fuzzer.go:526-532: new_k = Canonicalize(SignalDiff(corpusSignal, S_k)),
 * every input against the same corpusSignal (only read).  S_k = vals[off[k] ..
 * off[k+1]); new_vals capacity off[n]; new_off (n+1) gives each new_k. */
int sg_triage_newsig(sg_ctx* ctx, sg_set* corpus, const uint32_t* vals, const uint64_t* off, size_t n,
		     uint32_t* new_vals, uint64_t* new_off);
/* fuzzer.go:567: new_k = Intersection(new_k, Canonicalize(R_k)) for sorted new_k
 * (new_vals[new_off[k] ..]) and raw re-execution signal R_k (r_vals[r_off[k]
 * ..]); the result is written at new_k's own start, out_len[k] = its length. */
int sg_triage_intersect(sg_ctx* ctx, uint32_t* new_vals, const uint64_t* new_off, const uint32_t* r_vals,
			const uint64_t* r_off, size_t n, uint64_t* out_len);
/* fuzzer.go:584-587, the minimisation predicate: ok[k] =
 * len(Intersection(new_k, Canonicalize(R_k))) == len(new_k). */
int sg_triage_subset(sg_ctx* ctx, const uint32_t* new_vals, const uint64_t* new_off, const uint32_t* r_vals,
		     const uint64_t* r_off, size_t n, uint8_t* ok);

/* syz-manager/manager.go:907-912 NewInput() signal part, over n RPCs in
 * arrival order: accepted[k] = SignalNew(corpusSignal, S_k) at its turn; on
 * accept corpusSignal ∪= S_k and corpusCover ∪= Cov_k.  cover may be NULL. */
int sg_accept_batch(sg_ctx* ctx, sg_set* corpus_sig, sg_set* corpus_cov, const uint32_t* sig_vals,
		    const uint64_t* sig_off, const uint32_t* cov_vals, const uint64_t* cov_off, size_t n,
		    uint8_t* accepted);

/* syz-manager/manager.go:949-956 Poll() maxSignal merge over npoll polls in
 * arrival order: poll k's newMaxSignal = members of A_k not yet in maxSignal,
 * first occurrences, in A_k order.  new_vals capacity a_off[npoll]; new_off
 * (npoll+1) gives each poll's slice. */
int sg_merge_poll(sg_ctx* ctx, sg_set* mgr_max, const uint32_t* a_vals, const uint64_t* a_off, size_t npoll,
		  uint32_t* new_vals, uint64_t* new_off);

/* pkg/cover/cover.go:120-146 Minimize() over corpus CSR (vals/off, n inputs)
 * processed in `order` (order[k] = input index processed k-th; the reference
 * takes it from sort.Sort of minInputArray, cover.go:128).  out_idx gets the
 * selected input indices in processing order; *nout their count. */
int sg_minimize(sg_ctx* ctx, const uint32_t* vals, const uint64_t* off, size_t n, const uint32_t* order,
		uint32_t* out_idx, size_t* nout);
/* order of cover.Minimize: Go's sort.Sort over minInputArray (Less = longer
 * first, cover.go:157), restated from the Go 1.8/1.9 sort package. */
int sg_minimize_order(const uint64_t* off, size_t n, uint32_t* order);

/* ---- RPC payloads (pkg/rpctype/rpctype.go:8-63) --------------------------- */
/* Wire form of a sorted []uint32 (RpcInput.Signal / .Cover are canonical;
 * ConnectRes.MaxSignal, PollArgs.MaxSignal and PollRes.MaxSignal are set
 * members): Go's binary.PutUvarint of the first value, then of each successive
 * difference.  A Go peer decodes it with binary.Uvarint and a running sum.
 * Batched over n lists: list k is vals[off[k] .. off[k+1]) (non-decreasing,
 * else SG_EINVAL); its bytes go to out[out_off[k] .. out_off[k+1]).  out_off
 * (n+1) is always filled; the bytes are copied only when out_off[n] <= cap
 * (cap = 5 * off[n] always suffices). */
int sg_delta_encode_batch(sg_ctx* ctx, const uint32_t* vals, const uint64_t* off, size_t n, uint8_t* out, size_t cap,
			  uint64_t* out_off);
/* The inverse: list k from in[in_off[k] .. in_off[k+1]) into vals[off[k] ..)
 * (capacity cap values; in_off[n] always suffices).  SG_EINVAL on a malformed
 * payload (a list ending inside a value, a value or running sum past 32 bits). */
int sg_delta_decode_batch(sg_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t n, uint32_t* vals, size_t cap,
			  uint64_t* off);
/* A set's members (ascending) as one payload: fuzzer.go:358-364 (PollArgs.MaxSignal
 * from newSignal), manager.go:801-806 / :962 (ConnectRes / PollRes.MaxSignal).
 * *nbytes = payload size; bytes copied only when it is <= cap. */
int sg_set_encode(sg_set* set, uint8_t* out, size_t cap, size_t* nbytes);
/* SignalAdd of a decoded payload (fuzzer.go:146-151, :392-398); *count
 * (nullable) = values in it. */
int sg_set_decode_add(sg_set* set, const uint8_t* in, size_t nbytes, uint64_t* count);
/* tools/syz-execprog/execprog.go:159-177: the sancov file of each of n calls:
 * u64 0xC0BFFFFFFFFFFF64, then RestorePC(pc, 0xffffffff) (cover.go:23-25) per
 * cover PC, little-endian.  File k is out[8*(k + cov_off[k]) .. 8*(k+1 +
 * cov_off[k+1])) (out: 8*(n + cov_off[n]) bytes). */
int sg_sancov_batch(sg_ctx* ctx, const uint32_t* cov, const uint64_t* cov_off, size_t n, uint8_t* out);
/* (execprog.go:162-164 writes no file for a call without cover: such a call's
 * slice here is the 8-byte header alone.) */

/* ---- sorted-slice algebra (pkg/cover/cover.go:28-117) ---------------------- */
/* Canonicalize (cover.go:28-40): in place, *nout = canonical length. */
int sg_canonicalize(sg_ctx* ctx, uint32_t* v, size_t n, size_t* nout);
/* Batched Canonicalize of CSR segments in place: segment k is
 * vals[off[k] .. off[k+1]); its canonical form is written at its own start,
 * out_len[k] = its length (Go returns cov[:n], aliasing the input). */
int sg_canonicalize_batch(sg_ctx* ctx, uint32_t* vals, const uint64_t* off, size_t nseg, uint64_t* out_len);

#define SG_OP_DIFFERENCE 0 /* cover.go:42-49 */
#define SG_OP_SYMDIFF 1    /* cover.go:51-61 */
#define SG_OP_UNION 2      /* cover.go:63-70 */
#define SG_OP_INTERSECT 3  /* cover.go:72-79 */
/* op(a, b) for sorted a, b; out capacity na+nb; *nout = result length. */
int sg_merge(sg_ctx* ctx, int op, const uint32_t* a, size_t na, const uint32_t* b, size_t nb, uint32_t* out,
	     size_t* nout);
/* Batched op over npair pairs: pair k is a[a_beg[k] .. +a_len[k]) op
 * b[b_beg[k] .. +b_len[k]) (pairs may share b, e.g. one corpus signal);
 * result k is written at out[out_beg[k] ..) (capacity a_len[k]+b_len[k]),
 * out_len[k] = its length.  Arrays are host pointers; a/b/out too. */
int sg_merge_batch(sg_ctx* ctx, int op, const uint32_t* a, size_t a_total, const uint64_t* a_beg,
		   const uint64_t* a_len, const uint32_t* b, size_t b_total, const uint64_t* b_beg,
		   const uint64_t* b_len, size_t npair, uint32_t* out, size_t out_total, const uint64_t* out_beg,
		   uint64_t* out_len);
/* The manager's cover.Union folds (cov = Union(cov, inp.Cover) over inputs:
 * syz-manager/html.go:84 grouped by syscall, :94, :184, :306, and the
 * same-hash merge manager.go:916-917): for each group g < ngroups, the Union
 * (cover.go:63-70) of the sorted lists k with group[k] == g (group NULL: one
 * group of all n lists) -- every value with its largest count over those
 * lists, ascending, 0xFFFFFFFF dropped.  List k is vals[off[k] .. off[k+1]).
 * Group g's fold goes to out_vals[out_off[g] .. out_off[g+1]) (out_off:
 * ngroups+1; capacity cap >= off[n] always suffices). */
int sg_union_fold(sg_ctx* ctx, const uint32_t* vals, const uint64_t* off, size_t n, const uint32_t* group,
		  size_t ngroups, uint32_t* out_vals, size_t cap, uint64_t* out_off);
/* HasDifference (cover.go:106-117): *out = 1 iff a has an element (multiset,
 * no sentinel special case) not matched in b. */
int sg_has_difference(sg_ctx* ctx, const uint32_t* a, size_t na, const uint32_t* b, size_t nb, int* out);
/* Batched HasDifference over npair pairs laid out as in sg_merge_batch (pair
 * k: a[a_beg[k] .. +a_len[k]) against b[b_beg[k] .. +b_len[k]); pairs may
 * share b): out[k] = 1 iff that a has an element not matched in that b, else
 * 0.  Host pointers. */
int sg_has_difference_batch(sg_ctx* ctx, const uint32_t* a, size_t a_total, const uint64_t* a_beg,
			    const uint64_t* a_len, const uint32_t* b, size_t b_total, const uint64_t* b_beg,
			    const uint64_t* b_len, size_t npair, uint8_t* out);

/* ---- executor edge signal (executor/executor.h:389-401, :497-526) --------- */
/* Raw per-call u32 PC traces -> per-call signal, executor-exact: edge
 * sig = pc ^ hash(prev pc) (prev = 0 at each call start), filtered through the
 * executor's lossy 8192-slot / 4-probe dedup table, one fresh table per
 * program shared by its calls in call order.  Programs own calls
 * [prog_off[p], prog_off[p+1]); call c owns pcs[call_off[c] .. call_off[c+1]).
 * Output: sig_vals (capacity call_off[ncalls]) and sig_off (ncalls+1). */
int sg_exec_signal(sg_ctx* ctx, const uint32_t* pcs, const uint64_t* call_off, const uint64_t* prog_off,
		   size_t nprog, uint32_t* sig_vals, uint64_t* sig_off);
int sg_exec_signal_dev(sg_ctx* ctx, const uint32_t* d_pcs, const uint64_t* d_call_off, const uint64_t* d_prog_off,
		       uint64_t nprog, uint64_t ncalls, uint64_t npcs, uint32_t* d_sig_vals, uint64_t* d_sig_off);
/* The executor-exact lists of the queued calls only (syz-fuzzer/fuzzer.go:678-683
 * copies inf.Signal of a record only when it is queued for triage): after a
 * set-exact triage of the same traces (sg_triage_traces_dev, flags d_rec_new),
 * call c's list is exactly sg_exec_signal_dev's when d_rec_new[c] != 0 and
 * empty otherwise.  Each program runs its calls up to its last queued one (the
 * executor's table state at a call depends only on the calls before it);
 * programs without a queued call do not run.  Layout as sg_exec_signal_dev. */
int sg_exec_signal_queued_dev(sg_ctx* ctx, const uint32_t* d_pcs, const uint64_t* d_call_off,
			      const uint64_t* d_prog_off, uint64_t nprog, uint64_t ncalls, uint64_t npcs,
			      const uint8_t* d_rec_new, uint32_t* d_sig_vals, uint64_t* d_sig_off);
/* The fuzzer's step from host traces in one call: sg_triage_traces (flags and
 * set updates, set-exact) and the executor-exact signal lists of the queued
 * calls only (sg_exec_signal_queued_dev), the traces staged once.  Calls are
 * grouped into programs by prog_off (nprog + 1, prog_off[0] == 0; the
 * executor's dedup table is per program); rec_new[c] for every call; the
 * lists in sig_vals / sig_off (ncalls + 1) as sg_exec_signal's, empty for the
 * calls not queued (fuzzer.go:678-683 copies the signal of queued calls
 * only).  sig_vals capacity: call_off[ncalls] values. */
int sg_triage_traces_queued(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* pcs,
			    const uint64_t* call_off, const uint64_t* prog_off, size_t nprog, uint8_t* rec_new,
			    uint32_t* sig_vals, uint64_t* sig_off);

/* ---- executor comparisons (executor/executor.h:379-387, :621-673) ---------- */
/* The flag_collect_comps branch of handle_completion over a batch of raw
 * KCOV_TRACE_CMP buffers.  recs is the KCOV layout unchanged, four u64 per
 * record {type, arg1, arg2, pc} (kcov_comparison_t, executor.h:118-123); call c
 * owns records call_off[c] .. call_off[c+1], call_off[0] == 0.  Any u64 is
 * legal in every field.  Per call, calls independent:
 *  - std::sort under operator< (:384, :665-673): by (type, arg1, arg2) as full
 *    unsigned 64-bit values;
 *  - std::unique under operator== (:385, :659-663): one record of every run
 *    equal in those three fields (pc takes no part and is never written, so
 *    which one stays cannot be observed);
 *  - kcov_comparison_t::write per survivor (:386-387, :621-657).
 * comp_off (ncalls + 1) is the prefix sum of each call's comps_size.  comps
 * holds three u64 per kept comparison in sorted order, {type, arg1', arg2'},
 * arg' being what write() leaves in the struct (:632-645): sign-extended from
 * 8, 16 or 32 bits when type & 6 is 0, 2 or 4, unchanged when it is 6.  The
 * extension comes after sort and unique, as in the reference: two records
 * that differ only above the operand width stay two entries, in raw order.
 * word_off (ncalls + 1) / words are the u32 words write() emits, in order:
 * (uint32_t)type, then (uint32_t)arg1', (uint32_t)arg2' when (type & 6) != 6,
 * else the low and high halves of arg1' and of arg2' (:646-656).  Pass
 * word_off == NULL to skip the words.
 * This is the WRITER's layout: two operand words unless the size is 8.  The
 * reader of this reference snapshot takes two operand words when the size IS 8
 * (pkg/ipc/ipc_linux.go:272-289), and sg_ipc_comps keeps reading it that way.
 * The device consumers of the full-width comps triples are sg_comps_pairs and
 * sg_hints_from_kcov ("hint seeds" below).
 * Offsets are always filled; comps (capacity comps_cap, in triples) is written
 * only when comp_off[ncalls] <= comps_cap, words (capacity words_cap) only when
 * word_off[ncalls] <= words_cap (the convention of sg_ipc_comps); nrecs triples
 * and 5 * nrecs words always suffice.  Limits (SG_EINVAL): nrecs < 2^32,
 * ncalls < 2^31.  A call's word count is kept in 32 bits: a single call of more
 * than (2^32 - 1) / 5 records is not supported (a KCOV buffer holds 16,383).
 * A call whose distinct records exceed SG_EXEC_COMPS_FAST_CAP leaves the
 * one-workgroup shape for the general (radix sort) path; it is never truncated. */
#define SG_EXEC_COMPS_FAST_CAP 4096
int sg_exec_comps(sg_ctx* ctx, const uint64_t* recs, const uint64_t* call_off, size_t ncalls, uint64_t* comp_off,
		  uint64_t* comps, size_t comps_cap, uint64_t* word_off, uint32_t* words, size_t words_cap);
/* Device form (nrecs = call_off[ncalls]): every pointer is device memory,
 * stream-ordered.  A batch of more than SG_EXEC_COMPS_FAST_CAP records costs
 * one small device-to-host read (16 B, one wait): the records of the calls
 * that left the fast shape size the general path's workspace.  Smaller batches,
 * and option "exec_comps_path" = 0, read nothing. */
int sg_exec_comps_dev(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t nrecs,
		      uint64_t* d_comp_off, uint64_t* d_comps, uint64_t comps_cap, uint64_t* d_word_off,
		      uint32_t* d_words, uint64_t words_cap);

/* ---- executor cover (executor/executor.h:402-415) --------------------------- */
/* The flag_collect_cover branch of handle_completion over a batch of raw KCOV
 * buffers: what a triage execution returns as Cover (syz-fuzzer/fuzzer.go:540-542
 * sets FlagCollectCover, :708 always adds FlagDedupCover).  pcs is the KCOV
 * layout unchanged, one u64 per PC (th->cover_data[i]); call c owns
 * pcs[call_off[c] .. call_off[c+1]), call_off[0] == 0.  Any u64 is a legal PC.
 * Calls are independent.  cov_off (ncalls + 1) / cov (u32, capacity cov_cap):
 *  - dedup == 0 (:413-414): cov is (uint32_t)pcs[i] in trace order and cov_off
 *    equals call_off;
 *  - dedup == 1 (flag_dedup_cover, :405-410): std::sort ascending as unsigned
 *    64-bit values (:408), std::unique (:409), then the truncation (:411-414).
 * The truncation comes after the unique, as in the reference ("assuming that
 * they fit into 32-bits", :411-412): 0x1_0000_0010 and 0x2_0000_0010 stay two
 * entries, in u64 order, so a call's u32 list may hold repeats and need not be
 * ascending when its PCs differ above bit 31.
 * Offsets are always filled; cov is written only when cov_off[ncalls] <=
 * cov_cap; call_off[ncalls] values always suffice.  SG_EINVAL: a NULL ctx,
 * call_off or cov_off; pcs NULL with PCs present; cov NULL with cov_cap > 0;
 * call_off[0] != 0 or decreasing offsets; 2^32 PCs or more, 2^31 calls or
 * more; dedup > 1.  A KCOV buffer holds at most 65,535 PCs (kCoverSize,
 * executor_linux.cc:39, :310); longer calls are exact all the same.
 * A call whose distinct PCs exceed SG_EXEC_COVER_FAST_CAP leaves the
 * one-workgroup shape for the general (radix sort) path; it is never truncated
 * (option "exec_cover_path", counters "exec_cover_general" and
 * "exec_cover_fast_cap"). */
#define SG_EXEC_COVER_FAST_CAP 8192
int sg_exec_cover(sg_ctx* ctx, const uint64_t* pcs, const uint64_t* call_off, size_t ncalls, int dedup,
		  uint64_t* cov_off, uint32_t* cov, size_t cov_cap);
/* Device form (npcs = call_off[ncalls]): every pointer is device memory,
 * stream-ordered.  The offsets cannot be checked: each call's range is clamped
 * to npcs.  With dedup == 1 a batch of more than SG_EXEC_COVER_FAST_CAP PCs
 * costs one small device-to-host read (16 B, one wait): the PCs of the calls
 * that left the fast shape size the general path's workspace.  Smaller batches
 * (no call of theirs can be flagged), dedup == 0 and option "exec_cover_path"
 * = 0 read nothing.  The capacity is checked on the device. */
int sg_exec_cover_dev(sg_ctx* ctx, const uint64_t* d_pcs, const uint64_t* d_call_off, uint64_t ncalls, uint64_t npcs,
		      int dedup, uint64_t* d_cov_off, uint32_t* d_cov, uint64_t cov_cap);

/* ---- triage re-runs from raw buffers (syz-fuzzer/fuzzer.go:521-576) --------- */
/* triageInput's loop for n candidates from the raw KCOV buffers of their nruns
 * re-executions each (1..8; the reference runs 3).  corpus is corpusSignal (only
 * read); sig_vals / sig_off (n + 1) hold each candidate's inp.signal, raw;
 * call[k] is inp.call, minimized[k] inp.minimized.  Execution e = k * nruns + i
 * is run i of candidate k: its calls are prog_off[e] .. prog_off[e+1] (n * nruns
 * + 1 offsets), call c owns pcs[call_off[c] .. call_off[c+1]), u64 PCs as
 * sg_exec_cover's.  An execution with no calls, or with fewer than call[k] + 1
 * calls, is len(info) == 0.  Per run, by definition: Signal_i is call call[k]'s
 * list from sg_exec_signal on the execution's PCs truncated as (uint32_t)pc
 * (executor/executor.h:394), the dedup table fresh per execution and shared by
 * its calls in order; Cover_i is that call's list from sg_exec_cover with dedup
 * = 1.  Per candidate, exactly fuzzer.go:526-576:
 *  1. new = Canonicalize(SignalDiff(corpus, inp.signal)) (:527-532); empty:
 *     SG_TIN_NO_NEW.
 *  2. minimized (:543-552): cover is a copy of the first non-empty Cover_i,
 *     whatever Signal_i is (none: empty); SG_TIN_OK, new as in step 1.
 *  3. otherwise (:553-576), for i ascending: an empty execution or an empty
 *     Signal_i is skipped once and ends the candidate with SG_TIN_NOT_EXECUTED
 *     the second time (:558-565); else new = Intersection(new,
 *     Canonicalize(Signal_i)) (:567), an empty new ends it with SG_TIN_FLAKY
 *     (:568-570), and cover becomes a copy of Cover_i when it is empty, else
 *     Union(cover, Cover_i) (:571-575; pkg/cover/cover.go:63-102: a copy keeps a
 *     0xFFFFFFFF and Union drops it, and Union keeps each value at its largest
 *     count).  A candidate that survives every run is SG_TIN_OK.
 * status (n); new_off (n + 1) / new_vals and cov_off (n + 1) / cov_vals: both
 * lists are empty for every status but SG_TIN_OK.  Offsets are always filled;
 * each payload is written only when it fits its own capacity (sig_off[n] and
 * call_off[ncalls] values always suffice).  prog.Minimize's predicate over the
 * same raw buffers is sg_minimize_pred_from_kcov (below), which takes new_vals /
 * new_off as they are; the caller then sends RpcInput{Signal:
 * Canonicalize(inp.signal), Cover: cover} (:596-603).
 * A Cover_i that is not non-decreasing as u32 (PCs that differ above bit 31)
 * makes foreach order-dependent; such candidates are folded by the literal
 * two-pointer loop and stay exact (counter "triage_runs_wide": the candidates of
 * the last call that held such a list).  Option "exec_cover_path" applies.
 * SG_EINVAL: a NULL ctx, corpus (or one of another context), offsets or, with
 * candidates, call / minimized / status; values NULL where present; a payload
 * NULL with its capacity > 0; offsets that do not start at 0 or decrease; nruns
 * outside 1..8; 2^28 candidates, 2^31 calls, 2^32 PCs or signals or more.
 * The host form stages once and reads back the status and the offsets, then
 * the payloads. */
#define SG_TIN_OK 0
#define SG_TIN_NO_NEW 1       /* fuzzer.go:529-531 */
#define SG_TIN_NOT_EXECUTED 2 /* :560-562 */
#define SG_TIN_FLAKY 3        /* :568-570 */
int sg_triage_runs_from_kcov(sg_ctx* ctx, sg_set* corpus, const uint32_t* sig_vals, const uint64_t* sig_off, size_t n,
			     const uint32_t* call, const uint8_t* minimized, uint32_t nruns, const uint64_t* pcs,
			     const uint64_t* call_off, const uint64_t* prog_off, int32_t* status, uint64_t* new_off,
			     uint32_t* new_vals, size_t new_cap, uint64_t* cov_off, uint32_t* cov_vals, size_t cov_cap);
/* Device form (nsig = sig_off[n], ncalls = prog_off[n * nruns], npcs =
 * call_off[ncalls]): every pointer is device memory.  The offsets cannot be
 * checked and are trusted as sg_exec_signal_dev trusts its own.  Stream-ordered
 * but for the waits its stages already have, all before the first run: the
 * 16 bytes of sg_exec_cover_dev when the batch holds more than
 * SG_EXEC_COVER_FAST_CAP PCs (or with "exec_cover_path" = 0), the SignalDiff
 * offsets ((n + 1) * 8 bytes, as sg_triage_newsig: Canonicalize is planned on
 * the host) and Canonicalize's lengths, after which the state words go up.  No
 * host round trip between the runs or after them.  Its intermediates live in
 * the context's grow-only device staging buffer. */
int sg_triage_runs_from_kcov_dev(sg_ctx* ctx, sg_set* corpus, const uint32_t* d_sig_vals, const uint64_t* d_sig_off,
				 uint64_t n, uint64_t nsig, const uint32_t* d_call, const uint8_t* d_minimized,
				 uint32_t nruns, const uint64_t* d_pcs, const uint64_t* d_call_off,
				 const uint64_t* d_prog_off, uint64_t ncalls, uint64_t npcs, int32_t* d_status,
				 uint64_t* d_new_off, uint32_t* d_new_vals, uint64_t new_cap, uint64_t* d_cov_off,
				 uint32_t* d_cov_vals, uint64_t cov_cap);

/* ---- minimisation predicate from raw buffers (syz-fuzzer/fuzzer.go:578-591) - */
/* The closure triageInput hands to prog.Minimize (prog/mutation.go:256-450,
 * which calls it once per removable call and once per simplified argument),
 * for a batch of n attempts: one predicate call each, drawn from any number of
 * concurrent Minimize runs.  new_vals / new_off (ncand + 1) are the newSignal
 * lists, each sorted non-decreasing (canonical lists are the normal case:
 * sg_triage_runs_from_kcov's output); they are only read.  Attempt e tests list
 * cand[e] < ncand (many attempts may share a list, in any order) on call
 * call[e] (call1) of its execution, which owns calls prog_off[e] ..
 * prog_off[e+1] (n + 1 offsets); call c owns pcs[call_off[c] .. call_off[c+1]),
 * u64 PCs laid out as sg_triage_runs_from_kcov's.  By definition Signal_e is
 * call[e]'s list from sg_exec_signal on the execution's PCs truncated as
 * (uint32_t)pc, the dedup table fresh per execution and shared by its calls in
 * order.  status[e]:
 *  - SG_MP_NOT_EXECUTED (:580-582): the execution has fewer than call[e] + 1
 *    calls, or Signal_e is empty.  This comes first: an empty list against an
 *    empty Signal_e is not SG_MP_OK.
 *  - SG_MP_OK: sg_triage_subset(list, Signal_e) says 1, that is the list is
 *    strictly increasing, holds no 0xFFFFFFFF, and each of its values occurs in
 *    Signal_e (:584-590); an empty list is SG_MP_OK.
 *  - SG_MP_LOST (:587-589) otherwise; a list with a repeat or the sentinel always.
 * With maxsig (newsig nullable; newsig only with maxsig) execute()'s own check
 * (:665-691) runs first, over all calls of all attempts in batch order, exactly
 * as sg_triage_traces_dev on the truncated PCs: rec_new[c] for every call and
 * both set updates.  sig_off (ncalls + 1) / sig_vals are then laid out as
 * sg_triage_traces_queued's: the executor-exact list of every call that is
 * queued (rec_new[c] != 0) or selected (call[e] of its execution), an empty
 * list for every other call.  The executor runs once, up to the last such call
 * of each execution.  sig_off is always filled; sig_vals (capacity sig_cap) is
 * written only when sig_off[ncalls] <= sig_cap; call_off[ncalls] values always
 * suffice.  Without maxsig no set is read or written, only the selected calls
 * run, and rec_new / sig_off / sig_vals are ignored (they may be NULL).
 * SG_EINVAL: a NULL ctx, new_off, prog_off or call_off; with attempts, a NULL
 * cand, call or status; values or PCs NULL where present; a set of another
 * context; newsig without maxsig; with maxsig, a NULL sig_off, a NULL rec_new
 * with calls, or sig_vals NULL with sig_cap > 0; offsets that do not start at 0
 * or decrease; cand[e] >= ncand, or a list that is not sorted; attempts without
 * any list; 2^28 attempts, 2^31 calls, 2^32 lists, list values or PCs or more
 * (with maxsig also sg_triage_traces_dev's limits).  n == 0 is SG_OK.
 * The host form stages once and reads back the status, then with maxsig the
 * flags, the offsets and the lists. */
#define SG_MP_OK 0
#define SG_MP_NOT_EXECUTED 1 /* fuzzer.go:580-582 */
#define SG_MP_LOST 2         /* :587-589 */
int sg_minimize_pred_from_kcov(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* new_vals,
			       const uint64_t* new_off, size_t ncand, const uint32_t* cand, const uint32_t* call, size_t n,
			       const uint64_t* pcs, const uint64_t* call_off, const uint64_t* prog_off, int32_t* status,
			       uint8_t* rec_new, uint64_t* sig_off, uint32_t* sig_vals, size_t sig_cap);
/* Device form (nnew = new_off[ncand], ncalls = prog_off[n], npcs =
 * call_off[ncalls]): every pointer is device memory, e.g. d_new_vals / d_new_off
 * as sg_triage_runs_from_kcov_dev left them.  The offsets, cand and the lists'
 * order cannot be checked and are trusted as sg_exec_signal_dev trusts its
 * offsets (list ranges are clamped to nnew, cand to ncand - 1).  Stream-ordered:
 * it adds no host wait of its own.  The waits its stages have: with maxsig,
 * those of sg_triage_traces_dev (one small device-to-host read per record
 * slice for a batch of more than 2^24 calls); without maxsig none.  Its
 * intermediates (the truncated PCs, the marks and the lists: 8 bytes per PC,
 * 9 per call) live in the context's grow-only device staging buffer, which
 * waits for the stream only when it has to grow. */
int sg_minimize_pred_from_kcov_dev(sg_ctx* ctx, sg_set* maxsig, sg_set* newsig, const uint32_t* d_new_vals,
				   const uint64_t* d_new_off, uint64_t ncand, uint64_t nnew, const uint32_t* d_cand,
				   const uint32_t* d_call, uint64_t n, const uint64_t* d_pcs, const uint64_t* d_call_off,
				   const uint64_t* d_prog_off, uint64_t ncalls, uint64_t npcs, int32_t* d_status,
				   uint8_t* d_rec_new, uint64_t* d_sig_off, uint32_t* d_sig_vals, uint64_t sig_cap);

/* ---- synthetic Zipf traces (bench / test input generator) ----------------- */
/* Zipf(s) over `nranks` PC ranks mapped through a permutation seeded by
 * universe_seed (the "kernel text": shared by every batch) to
 * pc = 0x81000000 + 16*perm(rank); draws are counter-based
 * (splitmix64 of trace_seed and the global PC index), so any slice is
 * reproducible.  Fills d_pcs with nprog*calls*pcs_per_call PCs of programs
 * prog_base .. prog_base+nprog-1, program-major. */
int sg_gen_zipf_traces_dev(sg_ctx* ctx, uint64_t universe_seed, uint64_t trace_seed, double zipf_s, uint32_t nranks,
			   uint64_t prog_base, uint64_t nprog, uint32_t calls, uint32_t pcs_per_call, uint32_t* d_pcs);
/* A fuzzer's steady state: programs drawn from a fixed population of npop
 * programs (member m's trace is the one sg_gen_zipf_traces_dev gives program m
 * under trace seed pop_seed), re-executed with flaky coverage -- each PC is
 * replaced by a fresh Zipf draw with probability `noise`.  The member of
 * program p and its noise are counter-based in (trace_seed, p). */
int sg_gen_population_traces_dev(sg_ctx* ctx, uint64_t universe_seed, uint64_t pop_seed, uint64_t npop,
				 uint64_t trace_seed, double noise, double zipf_s, uint32_t nranks, uint64_t prog_base,
				 uint64_t nprog, uint32_t calls, uint32_t pcs_per_call, uint32_t* d_pcs);

/* ---- cover report (syz-manager/cover.go:91-103, :257-307) ----------------- */
/* pcs[i] = RestorePC(cov[i], base) - 5; returns the uncovered PC set of
 * uncoveredPcsInFuncs, ascending (the reference returns map order).
 * sym_start/sym_end sorted by start; all_pcs sorted (objdump call sites).
 * out capacity nall; *nout = count. */
int sg_cover_uncovered(sg_ctx* ctx, const uint32_t* cov, size_t ncov, uint32_t base, const uint64_t* sym_start,
		       const uint64_t* sym_end, size_t nsym, const uint64_t* all_pcs, size_t nall, uint64_t* out,
		       size_t* nout);

/* ---- cover report line tables (syz-manager/cover.go:91-120, :165-196) ------- */
/* The rest of the /cover page's set math: generateCoverHtml
 * (syz-manager/cover.go:91-120) symbolises the covered and the uncovered PCs
 * and fileSet (syz-manager/cover.go:165-196) folds the frames into per-file
 * line lists, all of it under mgr.mu (httpCover, syz-manager/html.go:169-194).
 * The frames of a PC depend on vmlinux alone and the PCs a report can ask
 * about are known at start-up (allCoverPCs, cover.go:64-89), so the caller
 * symbolises them once into a table that stays on the device; a report is
 * then one call with no addr2line in it.
 *
 * sg_cover_table_create: sym_start / sym_end / all_pcs are sg_cover_uncovered's
 * inputs under the same ordering conditions.  tab_pcs (sorted, unique) are the
 * symbolised PCs and must contain every all_pcs entry; the frames of
 * tab_pcs[j] are entries frame_off[j] .. frame_off[j+1] (frame_off has
 * ntab + 1 entries, also when ntab == 0) in `addr2line -afi` order, zero
 * frames being legal (symbolizer.go:173 drops "??" and line <= 0).  A frame is
 * (file id < nfiles, line > 0, func id < nfuncs).  The caller interns the
 * strings: fileSet compares File and Func by string, so equal strings MUST get
 * equal ids (and different strings different ids).  Everything is checked on
 * the host before the context is touched (SG_EINVAL, sg_last_error says
 * what): null pointers, a count or the frame total >= 2^32 - 1, symbol or PC
 * order, frame_off not starting at 0 or decreasing, an id out of range or
 * line 0, a call site that is not in tab_pcs.  The table owns its device
 * memory (as an sg_set its words), is immutable, belongs to `ctx` and must be
 * destroyed before it.  Every distinct (file, line) pair of the table is a
 * slot; sg_cover_table_slots returns their number, the capacity a report's
 * lines / covered need.
 *
 * sg_cover_lines: pcs[i] = RestorePC(cov[i], base) - 5; uncovered =
 * uncoveredPcsInFuncs(pcs) exactly as sg_cover_uncovered computes it (query
 * order kept); the covered frames are the frames of every pcs[i] (duplicates
 * change nothing).  fileSet: every covered frame sets files[file][line] = true
 * and funcs[func] = true; an uncovered frame is kept only if its func is in
 * funcs (inlined covered frames count) and then sets files[file][line] = false
 * unless the line is there already.  A PC can be both (overlapping symbols):
 * its lines are covered.  File f's list is lines[file_off[f] .. file_off[f+1]),
 * ascending, covered[] (1 / 0) alongside; a file with no entry gets an empty
 * range (the reference's map has no key for it).  file_seen (nfiles, nullable):
 * bit 0 = the file appears in a covered frame, bit 1 = in an uncovered frame
 * before the funcs filter -- what symbolize's path prefix (cover.go:358-372) is
 * taken over.  Prefix strings and HTML stay with the caller; note that the
 * reference's `prefix == ""` reset makes the prefix depend on frame order only
 * when file names share no first byte.  *ncovered_frames = the frames of the
 * distinct covered PCs found in the table: 0 is the reference's "does not have
 * debug info" error (cover.go:113-115).  missing (capacity ncov; for the set
 * form the set's size) receives the distinct covered PCs that are not in
 * tab_pcs, ascending, *nmissing of them: they take part in
 * uncoveredPcsInFuncs (which needs no symbols) and contribute no frames; when
 * there are any the caller symbolises them, builds a table that contains them
 * and calls again.  ncov == 0: all-empty outputs and SG_OK (the reference's
 * "No coverage data available" is the caller's).  Nothing past file_off[nfiles]
 * entries of lines / covered and *nmissing entries of missing is meaningful.
 *
 * sg_cover_lines_set: the same for the members of `cov` in ascending order --
 * the reference's canonical cover order -- e.g. the corpus cover that
 * sg_accept_batch maintains; nothing is uploaded. */
typedef struct sg_cover_table sg_cover_table;
int sg_cover_table_create(sg_ctx* ctx, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym,
			  const uint64_t* all_pcs, size_t nall, const uint64_t* tab_pcs, size_t ntab,
			  const uint64_t* frame_off, const uint32_t* frame_file, const uint32_t* frame_line,
			  const uint32_t* frame_func, uint32_t nfiles, uint32_t nfuncs, sg_cover_table** out);
void sg_cover_table_destroy(sg_cover_table* table);
int sg_cover_table_slots(sg_cover_table* table, uint64_t* nslots);
int sg_cover_lines(sg_cover_table* table, const uint32_t* cov, size_t ncov, uint32_t base, uint64_t* file_off,
		   uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames, uint64_t* missing,
		   size_t* nmissing);
int sg_cover_lines_set(sg_cover_table* table, sg_set* cov, uint32_t base, uint64_t* file_off, uint32_t* lines,
		       uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames, uint64_t* missing,
		       size_t* nmissing);

/* ---- cover report pages (syz-manager/cover.go:122-156, :198-217) ------------ */
/* The rest of generateCoverHtml up to its template: the loop over fileSet's
 * map (syz-manager/cover.go:122-156) reads every file of the report again on
 * every request (parseFile, syz-manager/cover.go:198-217) and writes every
 * line of it into a buffer, a listed line between one of two pairs of
 * literals -- still under mgr.mu (httpCover, syz-manager/html.go:169-194).
 * The sources depend on the tree alone, as the frames on vmlinux alone, so
 * the caller reads them once into a table that stays on the device; a report
 * is then one call from the cover to each file's Body and Coverage, the
 * templateFile of cover.go:151-155.  coverTemplate and its execution, the
 * prefix strip (cover.go:148-150) and the sort (cover.go:158) stay with the
 * caller.
 *
 * sg_src_table_create: file f is the sg_cover_table's file id f; its bytes are
 * bytes[off[f] .. off[f+1]).  have[f] == 0: the caller could not read it
 * (parseFile's error, cover.go:199-202) and its range must be empty.  The
 * table holds exactly parseFile's lines (cover.go:203-215): every stretch up
 * to a '\n' is a line and passes, byte by byte, through the replacer of
 * cover.go:203 ('>' "&gt;", '<' "&lt;", '&' "&amp;", '\t' eight spaces; no
 * second pass over what it wrote); what follows the file's last '\n', when not
 * empty, is one more line and is NOT escaped (cover.go:213-215 appends the raw
 * bytes); '\r', NUL and bytes >= 0x80 pass unchanged; an empty file has no
 * lines and "\n" one empty line.  Stored is the text with a '\n' behind every
 * line, the raw fragment included (cover.go:144-145 appends one to every
 * line): byte for byte the file's body when nothing is listed.  Checked on the
 * host before the context is touched (SG_EINVAL, sg_last_error says what):
 * null pointers, off not starting at 0 or decreasing, have[f] == 0 with a
 * non-empty range, 2^32 or more bytes; after the count phase 2^32 or more
 * stored bytes.  The table is immutable, belongs to `ctx` and must be
 * destroyed before it.
 *
 * sg_src_table_counts: file f's lines are file_line_off[f] ..
 * file_line_off[f+1] (nfiles + 1 entries) of the table's; totals = lines,
 * stored bytes, raw bytes.  sg_src_table_export: line i's text is
 * text[line_off[i] .. line_off[i+1] - 1) (lines + 1 offsets; the byte before
 * line_off[i+1] is the '\n'), text has totals[1] bytes.
 *
 * sg_cover_pages: everything up to nmissing means what it means for
 * sg_cover_lines and is checked the same way.  Then cover.go:123-147 runs for
 * every file with a non-empty range (the keys of fileSet's map), in file-id
 * order: the body is the file's lines in order, each followed by '\n'; a line
 * whose 1-based number is in the file's list stands between
 * "<span id='covered'>" and 20 bytes ("</span> ", a C comment of the word
 * covered, '\n': the suffix carries the '\n'; cover.go:133-135) or between
 * "<span id='uncovered'>" and "</span>\n" (cover.go:138-140).  Listed lines are > 0, distinct and ascending, so the
 * loop's covered[0] walk (cover.go:131, :142) wraps every listed line <= the
 * file's line count and silently drops one beyond it.  coverage[f] counts the
 * covered lines actually wrapped (cover.go:136); a file with no lines gets an
 * empty body and coverage 0.  File f's body is bodies[body_off[f] ..
 * body_off[f+1]) (nfiles + 1 offsets); a file outside the report has an empty
 * range.  *bad_file = the lowest id of a file of the report with have == 0,
 * else UINT32_MAX; when there is one nothing is rendered (*nbytes = 0,
 * body_off and coverage all 0), the return is still SG_OK and the line tables
 * are valid (the reference fails the page at the first such file in map
 * order, cover.go:124-127).  *nbytes is always the bodies' total; bodies
 * (capacity cap) is written only when the total is <= cap, body_off and
 * coverage always; bodies == NULL with cap > 0 is SG_EINVAL.  The bodies match
 * the line tables of the same call, also when *nmissing > 0.  ncov == 0:
 * all-empty outputs and SG_OK.  src and table must share a context and nfiles
 * (SG_EINVAL).  The call makes no more waits than sg_cover_lines, but one when
 * the context's output buffer has to grow for the bodies: body_off, coverage
 * and the total come back with its counts, the bodies with its lines.  Counter "cover_pages_tile": the bytes of the bodies one workgroup of
 * the copy writes.
 *
 * sg_cover_pages_set: the same for the members of `cov`, as
 * sg_cover_lines_set. */
typedef struct sg_src_table sg_src_table;
int sg_src_table_create(sg_ctx* ctx, const uint8_t* have, const uint8_t* bytes, const uint64_t* off, uint32_t nfiles,
			sg_src_table** out);
void sg_src_table_destroy(sg_src_table* src);
int sg_src_table_counts(sg_src_table* src, uint64_t* file_line_off, uint64_t totals[3]);
int sg_src_table_export(sg_src_table* src, uint64_t* line_off, uint8_t* text);
int sg_cover_pages(sg_cover_table* table, sg_src_table* src, const uint32_t* cov, size_t ncov, uint32_t base,
		   uint64_t* file_off, uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
		   uint64_t* missing, size_t* nmissing, uint64_t* body_off, uint32_t* coverage, uint8_t* bodies,
		   size_t cap, size_t* nbytes, uint32_t* bad_file);
int sg_cover_pages_set(sg_cover_table* table, sg_src_table* src, sg_set* cov, uint32_t base, uint64_t* file_off,
		       uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
		       uint64_t* missing, size_t* nmissing, uint64_t* body_off, uint32_t* coverage, uint8_t* bodies,
		       size_t cap, size_t* nbytes, uint32_t* bad_file);

/* ---- executor output ingest (pkg/ipc/ipc_linux.go:168-307) ---------------- */
/* readOutCoverage over a batch of programs.  Program p's output region (the
 * layout executor/executor.h:369-427 writes) is out[out_off[p] ..
 * out_off[p+1]); its calls are records call_off[p] .. call_off[p+1]
 * (len(p.Calls)); call_nums[r] = c.Meta.ID of record r, or NULL to skip that
 * check (ipc_linux.go:225-230).  Per record: err = Errno (-1 = not executed,
 * else the executor's u32 errno), fault = FaultInjected, its Signal words at
 * sig_vals[sig_off[r] .. sig_off[r+1]) and, when cov_off / cov_vals are
 * given, its Cover words likewise.  Comparisons are walked, not decoded.
 * status[p] = SG_IPC_OK or the Go error path the reader took; the records
 * keep what the reader had set before it (partial info, as in Go).
 * sig_vals / cov_vals capacity: out_off[nprog] words always suffices.
 * Record order is program-major, call index ascending (fuzzer.go:665). */
#define SG_IPC_OK 0
#define SG_IPC_NO_NCMD 1      /* ipc_linux.go:197-200 */
#define SG_IPC_SHORT_HEADER 2 /* :216-219 */
#define SG_IPC_BAD_INDEX 3    /* :220-224 */
#define SG_IPC_BAD_CALLNUM 4  /* :225-230 */
#define SG_IPC_DOUBLE 5       /* :231-235 */
#define SG_IPC_SIGNAL_SIZE 6  /* :238-242 */
#define SG_IPC_COVER_SIZE 7   /* :247-251 */
#define SG_IPC_COMPS_SHORT 8  /* :258-290 */
#define SG_IPC_COMPS_TYPE 9   /* :266-270 */
int sg_ipc_parse(sg_ctx* ctx, const uint32_t* out, const uint64_t* out_off, const uint64_t* call_off,
		 const uint32_t* call_nums, size_t nprog, int64_t* err, uint8_t* fault, int32_t* status,
		 uint64_t* sig_off, uint32_t* sig_vals, uint64_t* cov_off, uint32_t* cov_vals);
/* Device form: every pointer is device memory, stream-ordered, no host sync. */
int sg_ipc_parse_dev(sg_ctx* ctx, const uint32_t* d_out, const uint64_t* d_out_off, const uint64_t* d_call_off,
		     const uint32_t* d_call_nums, uint64_t nprog, uint64_t nrec, int64_t* d_errno, uint8_t* d_fault,
		     int32_t* d_status, uint64_t* d_sig_off, uint32_t* d_sig_vals, uint64_t* d_cov_off,
		     uint32_t* d_cov_vals);

/* ---- comparison hints (pkg/ipc/ipc_linux.go:257-304, prog/hints.go) ------- */
/* The comparison half of readOutCoverage over a batch of programs
 * (ipc_linux.go:257-304); out / out_off / call_off / call_nums as
 * sg_ipc_parse's.  A pair is two u64 {key, value}, one AddComp(key, value);
 * record r's pairs, pairs[2 * pair_off[r] .. 2 * pair_off[r+1]), are the
 * reader's AddComp calls for that call in the reader's order: per comparison
 * the type word (SG_IPC_COMPS_TYPE above 7), operands of two words when
 * (typ & 6) == 6 and of four words read as two little-endian u64 otherwise,
 * nothing when op1 == op2, else (op2, op1) and, when typ & 1 == 0, also
 * (op1, op2).  A call's CompMap is the set of its pairs; they are not
 * deduplicated here.  status[p] is what sg_ipc_parse returns for the same
 * region; a program whose status is not SG_IPC_OK gets empty lists for all
 * its records (as its signal does), and so do the calls that did not execute.
 * pair_off (nrec + 1) is always filled; pairs (capacity cap, in pairs) is
 * written only when pair_off[nrec] <= cap (the convention of
 * sg_delta_encode_batch); 2 * ceil(out_off[nprog] / 3) pairs always suffice.
 * A program's region holds at most 2^32 words (the reader's own view of the
 * output is 2^28). */
int sg_ipc_comps(sg_ctx* ctx, const uint32_t* out, const uint64_t* out_off, const uint64_t* call_off,
		 const uint32_t* call_nums, size_t nprog, int32_t* status, uint64_t* pair_off, uint64_t* pairs,
		 size_t cap);
/* Device form: every pointer is device memory, stream-ordered, no host sync.
 * d_pairs may be NULL when cap is 0 (the offsets alone). */
int sg_ipc_comps_dev(sg_ctx* ctx, const uint32_t* d_out, const uint64_t* d_out_off, const uint64_t* d_call_off,
		     const uint32_t* d_call_nums, uint64_t nprog, uint64_t nrec, int32_t* d_status,
		     uint64_t* d_pair_off, uint64_t* d_pairs, uint64_t cap);
/* shrinkExpand (prog/hints.go:150-177) over a batch: the loop bodies of
 * checkConstArg (:95-99) and checkDataArg (:101-118).  Record r's CompMap is
 * its pairs (pair_off / pairs as above); its argument values are
 * vals[val_off[r] .. val_off[r+1]): one slot per ConstArg.Val, and one per
 * window sliceToUint64(Data[i:]), i < min(len, 100), of a DataArg.  Slot i gets
 * the distinct members of shrinkExpand(vals[i], CompMap_r) at
 * reps[rep_off[i] .. rep_off[i+1]), ascending (the reference iterates a map).
 * rep_off (val_off[nrec] + 1) is always filled; reps (capacity cap) is
 * written only when rep_off[nvals] <= cap.  The number of slots, of pairs and
 * of (slot, pair) matches must each be below 2^32 (SG_EINVAL otherwise). */
int sg_hints_replacers(sg_ctx* ctx, const uint64_t* pair_off, const uint64_t* pairs, size_t nrec,
		       const uint64_t* val_off, const uint64_t* vals, uint64_t* rep_off, uint64_t* reps, size_t cap);
/* Device form (nvals = val_off[nrec]): stream-ordered but for one small
 * device-to-host read (about 1 KiB, one wait): the match count that sizes its
 * workspace and the replacers' varying bits. */
int sg_hints_replacers_dev(sg_ctx* ctx, const uint64_t* d_pair_off, const uint64_t* d_pairs, uint64_t nrec,
			   const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals, uint64_t* d_rep_off,
			   uint64_t* d_reps, uint64_t cap);

/* ---- hint seeds: raw comparisons to replacers (syz-fuzzer/fuzzer.go:627-643) */
/* The reader's loop body (pkg/ipc/ipc_linux.go:290-302) at full operand width
 * over a triples CSR, the layout sg_exec_comps returns: call c's comparisons
 * are the triples {type, arg1, arg2} comps[3 * comp_off[c] .. 3 * comp_off[c+1]),
 * comp_off[0] == 0.  Calls are independent.  Per triple, in order: op1, op2 are
 * arg1, arg2 sign-extended from 8, 16 or 32 bits when type & 6 is 0, 2 or 4,
 * unchanged when it is 6 (kcov_comparison_t::write, executor/executor.h:632-645;
 * idempotent, so a no-op on sg_exec_comps' output, and any triples are legal
 * input); nothing when op1 == op2 (:290-293), else the pair (op2, op1) (:294)
 * and, when type & 1 == 0, also (op1, op2) (:295-302).  A call that holds a
 * triple with type > 7 is the reader's :266-270 error: status[c] =
 * SG_IPC_COMPS_TYPE and an empty pair list (the reader assigns Comps after the
 * loop, :304); every other call has SG_IPC_OK and is unaffected.
 * status (ncalls) and pair_off (ncalls + 1) are always filled; pairs (two u64
 * {key, value} per pair, capacity cap in pairs, as sg_ipc_comps') is written
 * only when pair_off[ncalls] <= cap; 2 * comp_off[ncalls] pairs always suffice.
 * SG_EINVAL: a NULL ctx, comp_off, status or pair_off; comps NULL with
 * comparisons present; pairs NULL with cap > 0; comp_off[0] != 0 or decreasing
 * offsets; 2^31 comparisons or more (the pairs stay below 2^32), 2^31 calls or
 * more.  The host form stages its inputs once. */
int sg_comps_pairs(sg_ctx* ctx, const uint64_t* comp_off, const uint64_t* comps, size_t ncalls, int32_t* status,
		   uint64_t* pair_off, uint64_t* pairs, size_t cap);
/* Device form (ncomps = comp_off[ncalls]): every pointer is device memory,
 * stream-ordered, no host wait; the capacity is checked on the device.  The
 * offsets cannot be checked: they are clamped to ncomps. */
int sg_comps_pairs_dev(sg_ctx* ctx, const uint64_t* d_comp_off, const uint64_t* d_comps, uint64_t ncalls,
		       uint64_t ncomps, int32_t* d_status, uint64_t* d_pair_off, uint64_t* d_pairs, uint64_t cap);
/* A hint seed's raw KCOV_TRACE_CMP buffers and argument values to shrinkExpand's
 * replacers in one call.  recs / call_off are sg_exec_comps', val_off / vals /
 * rep_off / reps / cap are sg_hints_replacers' with record r being call r.  The
 * result is, by definition, that of sg_exec_comps on the buffers, sg_comps_pairs
 * on its triples and sg_hints_replacers on those pairs and the values; status
 * (ncalls) is sg_comps_pairs': a call with SG_IPC_COMPS_TYPE has an empty
 * CompMap, so all its slots get empty lists.  The triples and the pairs stay in
 * device memory; no triples and no words are written at all.  Option
 * "exec_comps_path" applies as in sg_exec_comps; the counters
 * "exec_comps_general" and "hints_candidates" report this call's stages.
 * SG_EINVAL: what the three stages reject (a NULL ctx, call_off, val_off, status
 * or rep_off; recs / vals NULL with records / values present; reps NULL with
 * cap > 0; offsets that do not start at 0 or decrease; 2^31 calls or 2^32 value
 * slots or (slot, pair) matches or more), and 2^31 records or more: a call keeps
 * at most its records, and the pairs of 2^31 comparisons could reach 2^32.
 * The host form copies the buffers, offsets and values in once, reads the
 * status and the offsets back, then the replacers when they fit. */
int sg_hints_from_kcov(sg_ctx* ctx, const uint64_t* recs, const uint64_t* call_off, size_t ncalls,
		       const uint64_t* val_off, const uint64_t* vals, int32_t* status, uint64_t* rep_off, uint64_t* reps,
		       size_t cap);
/* Device form (nrecs = call_off[ncalls], nvals = val_off[ncalls]): every pointer
 * is device memory, stream-ordered but for the two small device-to-host reads
 * its stages already have: sg_exec_comps_dev's 16 bytes when the batch holds
 * more than SG_EXEC_COMPS_FAST_CAP records (none with "exec_comps_path" = 0),
 * and sg_hints_replacers_dev's match count (about 1 KiB).  Its intermediates
 * (2 * nrecs pairs, two offsets per call) live in the context's grow-only
 * device staging buffer, which waits for the stream only when it has to grow. */
int sg_hints_from_kcov_dev(sg_ctx* ctx, const uint64_t* d_recs, const uint64_t* d_call_off, uint64_t ncalls,
			   uint64_t nrecs, const uint64_t* d_val_off, const uint64_t* d_vals, uint64_t nvals,
			   int32_t* d_status, uint64_t* d_rep_off, uint64_t* d_reps, uint64_t cap);

/* ---- call priorities: corpus to ChoiceTable (prog/prio.go:27-36, :133-229) -- */
/* What Manager.Connect computes between minimizeCorpus and the maxSignal export
 * (syz-manager/manager.go:816-837: target.CalculatePriorities(corpus), at most
 * every 30 minutes because it is slow), what the /prio page shows a row of
 * (syz-manager/html.go:196-224, mgr.prios as last computed), and what every
 * fuzzer makes of the matrix (prog/prio.go:203-229, BuildChoiceTable), from the
 * programs' call ids.
 *
 * Input: a CSR of Call.Meta.ID.  Program p owns call_ids[prog_off[p] ..
 * prog_off[p+1]), prog_off[0] == 0.  ncalls is len(target.Syscalls); mmap_id is
 * target.MmapSyscall.ID, or SG_NO_CALL for a target without one.
 *
 * Counts (prog/prio.go:138-151): count[i][j] = sum over programs of
 * n_p(i) * n_p(j) for i != j, i != mmap_id, j != mmap_id, with n_p(i) the calls
 * of program p with id i (both loops run over p.Calls, repeats included).  The
 * table keeps them exact, as 64-bit integers.  The reference adds 1.0 to a
 * float32, which is exact up to 2^24 and then sticks, so its cell is
 * float32(min(count, 2^24)): the saturation is applied when the counts are
 * read (sg_call_prios*), never when they are accumulated, and
 * sg_prio_table_counts returns them unsaturated.
 *
 * normalizePrio (prog/prio.go:158-192) per row, every operation rounded to
 * float32 in the reference's order: max over the row; min over the nonzero
 * cells from 1e10; nzero, and min /= 2 * float32(nzero) when nzero != 0; a row
 * with max == 0 becomes all 1; otherwise a zero cell takes min, and
 * p = (p - min) / (max - min) * 0.9 + 0.1 (float32 constants; the multiply and
 * the add are two roundings: Go on amd64 does not fuse them), clamped to 1.
 * The diagonal of the counts is always zero, so nzero >= 1 in every row and
 * max > min whenever max > 0: no NaN can arise.  That is `dynamic`.
 *
 * CalculatePriorities (prog/prio.go:27-36): prios[i][j] = dynamic[i][j] *
 * static[i][j], one float32 multiply.  The static matrix is an input: it
 * depends on the target alone, and the reference sums it in Go map order
 * (prog/prio.go:106-116), so its last bits differ from run to run in the
 * reference itself.  The caller computes it once.
 *
 * BuildChoiceTable (prog/prio.go:203-229): for an enabled row i,
 * run[i][j] = sum over k <= j with enabled[k] of int(prios[i][k] * 1000), the
 * product rounded to float32, then truncated.  A disabled row (nil in Go) is
 * all zeros.  enabled == NULL enables every call.  run is int32: the largest
 * sum is 1000 * ncalls.
 *
 * All matrices are row-major, ncalls * ncalls. */
#define SG_NO_CALL 0xffffffffu
#define SG_PRIO_MAX_CALLS 8192
typedef struct sg_prio_table sg_prio_table;
/* The table owns one device block: the static matrix, the enabled bytes and
 * the 64-bit counts (zero at creation).  It lives in ctx and must be destroyed
 * before it.  static_prios (ncalls * ncalls) and enabled (ncalls bytes, nonzero
 * = enabled, nullable) are copied.  SG_EINVAL, before the context is touched: a
 * NULL ctx, static_prios or out; ncalls == 0 or above SG_PRIO_MAX_CALLS;
 * mmap_id >= ncalls unless it is SG_NO_CALL; a static value that is not finite
 * or not in [0, 1].  SG_ENODEV without a device. */
int sg_prio_table_create(sg_ctx* ctx, uint32_t ncalls, uint32_t mmap_id, const float* static_prios,
			 const uint8_t* enabled, sg_prio_table** out);
void sg_prio_table_destroy(sg_prio_table* t);
/* All counts to zero (stream-ordered). */
int sg_prio_table_clear(sg_prio_table* t);
/* Adds a corpus' pairs to the counts: two adds equal one add of the
 * concatenation.  Programs may have any length, zero included.  SG_EINVAL,
 * before the context is touched: a NULL t or prog_off; prog_off[0] != 0 or
 * decreasing offsets; 2^32 ids or more; call_ids NULL with ids present; an id
 * >= ncalls.  Returns once the arrays are the caller's again.
 * Removing programs is left out: a removal cannot be validated against what
 * was added.  After minimizeCorpus the caller clears and re-adds. */
int sg_prio_table_add(sg_prio_table* t, const uint32_t* call_ids, const uint64_t* prog_off, size_t nprogs);
/* Device form (nids = the ids in d_call_ids): every pointer is device memory,
 * stream-ordered, nothing is read back.  The offsets cannot be checked: every
 * program's range is clamped to nids.  An id >= ncalls is skipped, never used
 * as an index, and counted in the context counter "prio_bad_ids".  SG_EINVAL:
 * a NULL t or d_prog_off, d_call_ids NULL with nids > 0, nids >= 2^32. */
int sg_prio_table_add_dev(sg_prio_table* t, const uint32_t* d_call_ids, const uint64_t* d_prog_off, uint64_t nprogs,
			  uint64_t nids);
/* The exact counts (ncalls * ncalls); waits. */
int sg_prio_table_counts(sg_prio_table* t, uint64_t* counts);
/* dynamic, prios and run (each ncalls * ncalls, each may be NULL) from the
 * counts, which stay unchanged.  One wait. */
int sg_call_prios(sg_prio_table* t, float* dynamic, float* prios, int32_t* run);
/* Device form: stream-ordered, no wait. */
int sg_call_prios_dev(sg_prio_table* t, float* d_dynamic, float* d_prios, int32_t* d_run);
/* sg_prio_table_clear, sg_prio_table_add and sg_call_prios in one call, with
 * one wait: what Connect and the /prio page need.  Rejects what add rejects;
 * on SG_EINVAL the counts are unchanged. */
int sg_call_prios_from_progs(sg_prio_table* t, const uint32_t* call_ids, const uint64_t* prog_off, size_t nprogs,
			     float* dynamic, float* prios, int32_t* run);

/* ---- program identities: pkg/hash and hubSync's Add / Del ------------------ */
/* pkg/hash (hash.Hash, hash.String) is SHA-1 of the serialized program, and
 * the reference recomputes it for the whole corpus under mgr.mu: hubSync
 * (syz-manager/manager.go:994-1069: at connect :1021-1025, per sync :1053-1056,
 * the diff against mgr.hubCorpus :1057-1069), minimizeCorpus (:777-781, and its
 * sweep of corpusDB.Records :788-793), NewInput (:913), the fuzzer's addInput
 * (syz-fuzzer/fuzzer.go:480-484) and the hub's loadDB (syz-hub/state/state.go:
 * 91-101).
 *
 * Input: a CSR of bytes.  Program k owns bytes[off[k] .. off[k+1]), off[0] == 0.
 * sigs[20 * k .. 20 * k + 20) is its SHA-1 (FIPS 180-4, what Go's crypto/sha1
 * computes; the padding's message length is a 64-bit bit count and is computed
 * as one).  hash.Hash(pieces...) hashes the concatenation of its pieces: the
 * caller joins them.
 *
 * A program longer than SG_SHA1_LONG bytes takes a path of its own (a wave to
 * itself); the context counter "sha1_long_progs" counts them, "sha1_long_len"
 * is the constant. */
#define SG_SIG_BYTES 20
#define SG_SHA1_LONG 65536
/* hash.Hash (sigs) and hash.String (hex: hex.EncodeToString, lower case, 40
 * characters per program, no NUL) of every program; either output may be NULL.
 * nprogs == 0 is SG_OK and writes nothing.  SG_EINVAL, before the context is
 * touched: a NULL ctx or off; off[0] != 0 or decreasing offsets; bytes NULL
 * with bytes present; 2^32 programs or more.  SG_ENODEV without a device.  One
 * wait. */
int sg_prog_hashes(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs, char* hex);
/* Device form (nbytes = the bytes in d_bytes): every pointer is device memory,
 * stream-ordered, nothing is read back.  The offsets cannot be checked: each
 * program's start is clamped to nbytes and its end to [start, nbytes], so
 * garbage offsets give garbage hashes, never a read outside [d_bytes, d_bytes +
 * nbytes).  SG_EINVAL: a NULL ctx, d_off or d_sigs with nprogs > 0; d_bytes
 * NULL with nbytes > 0; nprogs >= 2^32. */
int sg_prog_hashes_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs, uint64_t nbytes,
		       uint8_t* d_sigs);

/* map[hash.Sig]bool, device-resident: the fuzzer's corpusHashes (syz-fuzzer/
 * fuzzer.go:480-484), the manager's hubCorpus (manager.go:1021-1025).
 *
 * The set is insertion-ordered: sg_sigset_export returns the identities in the
 * order in which they first entered, which is batch order within a call.  The
 * reference's own order is Go map iteration, which is random; insertion order
 * is this project's pinned choice, not a parity claim.
 *
 * Inside: a dense store of 20-byte keys in insertion order, and an open-
 * addressing table of u32 indices into it with a power-of-two number of slots,
 * at most half of them used.  A key's home slot is its first four bytes read
 * as a little-endian u32, masked to the table.  The empty marker is an index
 * value (0xffffffff), never a key value: the all-zero and the all-0xff identity
 * are ordinary keys.  The set grows; capacity_hint only sizes the first
 * allocation.  A set holds fewer than 2^31 identities. */
typedef struct sg_sigset sg_sigset;
/* The set lives in ctx and must be destroyed before it.  SG_EINVAL, before
 * the context is touched: a NULL ctx or out, a hint of 2^31 or more.
 * SG_ENODEV without a device. */
int sg_sigset_create(sg_ctx* ctx, uint64_t capacity_hint, sg_sigset** out);
void sg_sigset_destroy(sg_sigset* s);
/* Empties the set; its allocations stay. */
int sg_sigset_clear(sg_sigset* s);
/* len(map).  No device work: the count is kept on the host. */
int sg_sigset_count(sg_sigset* s, uint64_t* out);
/* The identities in insertion order, 20 bytes each; *n is always the count, the
 * identities are written only when it is <= cap (in identities).  SG_EINVAL: a
 * NULL s or n, sigs NULL with cap > 0. */
int sg_sigset_export(sg_sigset* s, uint8_t* sigs, size_t cap, size_t* n);
/* present[k] = 1 iff sigs[20 * k ..) is in the set; reads only.  It serves
 * minimizeCorpus' sweep of corpusDB.Records (manager.go:788-793) and loadDB's
 * check (state.go:91-101).  SG_EINVAL: a NULL s, or sigs or present NULL with
 * n > 0; 2^31 queries or more. */
int sg_sigset_contains(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* present);
/* addInput's test (fuzzer.go:480-484) over a batch: is_new[k] = 1 iff sigs[k]
 * was not in the set before the call and no j < k of the batch has the same 20
 * bytes.  Afterwards the set is the union, the new identities appended in
 * batch order.  SG_EINVAL as sg_sigset_contains; also when the set would reach
 * 2^31 identities. */
int sg_sigset_add_new(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* is_new);
/* sg_prog_hashes followed by sg_sigset_add_new in one call with one wait; the
 * hashes leave the device only when sigs is given.  Rejects what both reject. */
int sg_sigset_add_progs(sg_sigset* s, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs,
			uint8_t* is_new);
/* hubSync's diff (manager.go:1053-1069) for a corpus given in a fixed order.
 * add[k] = 1 iff the hash of program k is neither in hub before the call nor
 * the hash of an earlier program of the call (a.Add, :1057-1061).  del_sigs
 * holds the identities that were in hub before the call and that no program
 * hashes to, in the set's order, *ndel of them (a.Del, :1063-1069).
 * Afterwards hub holds exactly the corpus' identities, in first-occurrence
 * program order (mgr.hubCorpus after :1061 and :1068).  An empty corpus deletes
 * everything.  del_cap (in identities) must be at least the set's count before
 * the call, which sg_sigset_count returns: otherwise SG_EINVAL before any
 * work, the set untouched.  SG_EINVAL also for what sg_prog_hashes rejects, a
 * NULL hub, add (with nprogs > 0) or ndel, del_sigs NULL with del_cap > 0.
 * sigs (20 * nprogs, may be NULL) receives the hashes.  Inside, a fresh table
 * and store are built from the corpus and swapped in: nothing is ever deleted
 * from a table, so there are no tombstones. */
int sg_hub_sync(sg_sigset* hub, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* sigs, uint8_t* add,
		uint8_t* del_sigs, size_t del_cap, size_t* ndel);

/* ---- the hub's corpus: prog.CallSet, pendingInputs, purgeCorpus ------------ */
/* syz-hub/state/state.go keeps the union of all managers' corpora, and under
 * the hub's lock State.Sync (state.go:175-195) walks all of it for every
 * manager's every sync: pendingInputs (state.go:265-308) tests rec.Seq, probes
 * the manager's corpus map and re-parses every record's text with prog.CallSet
 * (prog/encoding.go:559-592); purgeCorpus (state.go:338-354) rebuilds a `used`
 * map from every manager's corpus and sweeps the hub's; addInputs (state.go:
 * 310-336) parses, hashes and probes two maps per program; loadDB (state.go:
 * 83-110) does CallSet and the hash check over the whole database.
 *
 * prog.CallSet, pinned (encoding.go:559-592 over bufio.Scanner / ScanLines).  A
 * text is split at '\n'; the bytes after the last '\n' are a line only if there
 * are any; one trailing '\r' is dropped from each line; a line that is then
 * empty, or whose first byte is '#', is skipped.  Of any other line, bracket is
 * the first '(' and call = ln[:bracket]; if call contains '=', it starts after
 * the first '=' and after every ' ' (0x20 only, not a tab) that follows it.  The
 * name is exactly those bytes: trailing blanks, tabs, NUL and bytes >= 0x80 are
 * all part of it.  A program's status is its first failure in line order:
 *   SG_CALLSET_OK 0; SG_CALLSET_NO_BRACKET 1 "line does not contain opening
 *   bracket"; SG_CALLSET_EMPTY_NAME 2 "call name is empty"; SG_CALLSET_TOO_LONG
 *   3 the scanner's ErrTooLong; SG_CALLSET_NO_CALLS 4 "program does not contain
 *   any calls" (no failure and no call line).
 * Too long: the scanner's buffer limit is maxLineLen = 256 << 10 (encoding.go:
 * 382).  As bufio.Scanner.Scan is read here, a line fails exactly when its
 * content -- the bytes before its '\n', or before the end of the text, the
 * '\r' counted -- is SG_CALLSET_MAX_LINE bytes or more, whichever of the two
 * ends it; it fails when the scan reaches it, so an earlier line's status 1 or
 * 2 wins and a later one's does not.  That boundary is read, not run (Go is
 * not needed to build or test this library): parity unpinned at this edge. */
#define SG_CALLSET_OK 0
#define SG_CALLSET_NO_BRACKET 1
#define SG_CALLSET_EMPTY_NAME 2
#define SG_CALLSET_TOO_LONG 3
#define SG_CALLSET_NO_CALLS 4
#define SG_CALLSET_MAX_LINE 262144

/* The name dictionary: an exact interning table of call names (byte strings of
 * any length >= 1), ids dense in order of first insertion.  It is built on the
 * host (a target has a few thousand names): open addressing over ids, a power-
 * of-two number of slots, at most half of them used, a name's home slot the low
 * bits of its 64-bit FNV-1a hash with the constants below, which the kernel
 * shares.  The device holds a mirror (name bytes, name offsets, the 64-bit
 * hashes, the slots), uploaded again after every add that added.  Equality is
 * always decided by comparing the bytes; the stored hash only spares most
 * mismatches the byte compare. */
#define SG_FNV64_OFFSET 0xcbf29ce484222325ull
#define SG_FNV64_PRIME 0x100000001b3ull
#define SG_NAME_UNKNOWN 0xffffffffu
typedef struct sg_nametab sg_nametab;
/* SG_EINVAL: a NULL ctx or out.  SG_ENODEV without a device. */
int sg_nametab_create(sg_ctx* ctx, sg_nametab** out);
void sg_nametab_destroy(sg_nametab* t);
int sg_nametab_count(sg_nametab* t, uint64_t* out);
/* ids[k] = the id of name k = bytes[off[k] .. off[k+1]), an existing name
 * keeping its id.  SG_EINVAL, nothing added: a NULL t, ids NULL with n > 0, what
 * sg_prog_hashes rejects of a CSR, an empty name. */
int sg_nametab_add(sg_nametab* t, const uint8_t* bytes, const uint64_t* off, size_t n, uint32_t* ids);

/* prog.CallSet (encoding.go:559-592) of every program of a CSR of texts, as
 * each program's call lines in text order, repeats kept -- which is also what
 * PrioTable.add takes.  status[k] as above.  Program k owns call lines
 * line_off[k] .. line_off[k+1]; a program with status != 0 owns none.  Of call
 * line i, name_pos[i] is the name's byte offset into `bytes`, name_len[i] its
 * length and name_id[i] (nullable) its id in tab, SG_NAME_UNKNOWN for a name
 * that is not in it and for every line when tab is NULL.  *nlines is always
 * the total; the three arrays are written only when it is <= cap.  The number
 * of '(' bytes in the batch always suffices as cap.  SG_EINVAL, before the
 * context is touched: a NULL ctx, line_off or nlines, status NULL with nprogs
 * > 0, name_pos or name_len NULL with cap > 0, a tab of another context, what
 * sg_prog_hashes rejects of the CSR, 2^33 bytes of text or more.  SG_ENODEV
 * without a device.  Two waits. */
int sg_call_sets(sg_ctx* ctx, sg_nametab* tab, const uint8_t* bytes, const uint64_t* off, size_t nprogs, uint8_t* status,
		 uint64_t* line_off, uint64_t* name_pos, uint32_t* name_len, uint32_t* name_id, size_t cap,
		 size_t* nlines);
/* Device form: every pointer is device memory (tab stays the handle), stream-
 * ordered, nothing is read back; d_line_off[nprogs] is the total, and the
 * arrays are written only when it is <= cap.  The offsets follow
 * sg_prog_hashes_dev's rule: each start is clamped to nbytes and each end to
 * [start, nbytes]; garbage offsets give garbage lines, never a read outside
 * [d_bytes, d_bytes + nbytes).  With offsets that make programs overlap the
 * '(' count no longer bounds the total. */
int sg_call_sets_dev(sg_ctx* ctx, sg_nametab* tab, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nprogs,
		     uint64_t nbytes, uint8_t* d_status, uint64_t* d_line_off, uint64_t* d_name_pos, uint32_t* d_name_len,
		     uint32_t* d_name_id, uint64_t cap);

/* mgr.Corpus.Delete(sig) over a batch (state.go:181-183): removed[k] = 1 iff
 * sigs[k] was in the set and no j < k of the batch has the same 20 bytes.
 * Afterwards the set is without them, the rest in their old order.  A fresh
 * table and store are built from the survivors and swapped in, as sg_hub_sync
 * does: no tombstones.  SG_EINVAL as sg_sigset_contains. */
int sg_sigset_remove(sg_sigset* s, const uint8_t* sigs, size_t n, uint8_t* removed);

/* st.Corpus on the device.  A record is (key, seq, call ids): the keys live in
 * an identity set (sg_sigset's store and table), a record's index is its
 * store index, so records are in insertion order; seq[] and a CSR of each
 * record's call ids (line order, repeats kept) run parallel to it.  The texts
 * stay in the host's database: the calls return keys.  Deletion rebuilds
 * (gathered keys, seqs and ids, a fresh table), as sg_hub_sync does.
 * Orders are insertion order and (seq, record index): the reference's are Go
 * map iteration and an unstable sort, so these are pinned choices, not a parity
 * claim; the selected sets, max_seq and more are parity.
 * A seq is below SG_HUB_SEQ_LIMIT = 2^33: pending orders (seq << 31 | record
 * index) keys with radix_sort_u64, and a corpus holds fewer than 2^31 records. */
#define SG_HUB_SEQ_LIMIT (1ull << 33)
typedef struct sg_hubcorpus sg_hubcorpus;
/* The corpus lives in ctx, takes its ids from tab (of the same ctx), and must be
 * destroyed before both.  SG_EINVAL: a NULL argument, a tab of another context. */
int sg_hubcorpus_create(sg_ctx* ctx, sg_nametab* tab, sg_hubcorpus** out);
void sg_hubcorpus_destroy(sg_hubcorpus* h);
int sg_hubcorpus_count(sg_hubcorpus* h, uint64_t* nrecs);
/* Keys (20 bytes each), seqs, call_off (*nrecs + 1) and call_ids of all
 * records, in record order.  *nrecs and *nids are always the counts; the arrays
 * are written only when *nrecs <= cap_recs and *nids <= cap_ids. */
int sg_hubcorpus_export(sg_hubcorpus* h, uint8_t* sigs, uint64_t* seqs, uint64_t* call_off, uint32_t* call_ids,
			size_t cap_recs, size_t cap_ids, size_t* nrecs, size_t* nids);
/* addInputs' loop (state.go:314-317, :326-336) and loadDB's (:91-105).
 * status[k] is program k's CallSet status.  *nunk is the number of call lines
 * of status-0 programs whose name is not in the dictionary.  If *nunk > 0
 * NOTHING changes, neither the corpus nor mgr: the first min(*nunk, unk_cap)
 * spans (offset into bytes, length) are written in text order, the caller
 * interns them with sg_nametab_add and calls again.  So every stored record's
 * ids are known ids for good: no cached SG_NAME_UNKNOWN can go stale when a
 * later manager brings the name -- that is the reason for this protocol.
 * Otherwise, for each status-0 program in batch order: its SHA-1 enters mgr
 * (nullable; sg_sigset_add_new's semantics; :332); if it is neither in the
 * corpus nor an earlier program's of the batch it is appended with seqs[k] and
 * its ids (:333-335), and is_new[k] says so.  Programs with status != 0 are
 * skipped (:327-330, :92-96).  sigs (nullable) receives all nprogs hashes.
 * SG_EINVAL, before the context is touched: a NULL h, nunk, or with nprogs > 0
 * seqs, status or is_new; unk_pos or unk_len NULL with unk_cap > 0; a mgr of
 * another context; what sg_call_sets rejects of the CSR; a seqs value of
 * SG_HUB_SEQ_LIMIT or more; the corpus or mgr would reach 2^31 records. */
int sg_hubcorpus_add(sg_hubcorpus* h, sg_sigset* mgr, const uint8_t* bytes, const uint64_t* off, size_t nprogs,
		     const uint64_t* seqs, uint8_t* status, uint8_t* is_new, uint8_t* sigs, uint64_t* unk_pos,
		     uint32_t* unk_len, size_t unk_cap, size_t* nunk);
/* pendingInputs (state.go:265-308); reads only.  With mgr_seq == hub_seq: *n =
 * 0, *more = 0, *max_seq = hub_seq (the early return, :266-268).  Otherwise the
 * records with seq > mgr_seq, key not in mgr, and every call id's bit set in
 * mask (nwords 64-bit words; an id at or beyond 64 * nwords is not supported)
 * are selected; *max_seq = hub_seq, *more = 0; and if more than max_records
 * were selected they are ordered by seq, pos = max_records, *max_seq =
 * seq[pos], pos extends over equal seqs, pos++, *more = len - pos and [0, pos)
 * is kept (:286-300; index max_records is record number max_records + 1).
 * Output: keys and seqs in ascending (seq, record index) order.  *n is always
 * the count; the arrays are written only when it is <= cap; the corpus' count
 * always suffices.  SG_EINVAL: a NULL h, mgr, n, max_seq or more; mask NULL with
 * nwords > 0; sigs or seqs NULL with cap > 0; a mgr of another context. */
int sg_hubcorpus_pending(sg_hubcorpus* h, sg_sigset* mgr, uint64_t mgr_seq, uint64_t hub_seq, const uint64_t* mask,
			 size_t nwords, uint64_t max_records, uint8_t* sigs, uint64_t* seqs, size_t cap, size_t* n,
			 uint64_t* max_seq, uint64_t* more);
/* purgeCorpus (state.go:338-354): every record whose key is in none of the
 * nmgrs sets is deleted (nmgrs == 0 deletes all); the rest keep their order.
 * del_sigs receives the deleted keys in record order.  del_cap below the
 * corpus' count is SG_EINVAL before any work; so are a NULL h or ndel, mgrs
 * NULL (or a NULL or foreign entry) with nmgrs > 0, del_sigs NULL with del_cap
 * > 0. */
int sg_hubcorpus_purge(sg_hubcorpus* h, sg_sigset* const* mgrs, size_t nmgrs, uint8_t* del_sigs, size_t del_cap,
		       size_t* ndel);

/* ---- the corpus database: db.Open and loadDB from the file bytes ------------ */
/* pkg/db (pkg/db/db.go:38-52 Open, :125-131 the constants, :167-249
 * deserializeDB / deserializeHeader / deserializeRecord) reads a database
 * record by record and inflates every value on one thread through
 * compress/flate; the hub's loadDB (syz-hub/state/state.go:83-110) and the
 * manager's start-up (syz-manager/manager.go:178-216) wait for it before they
 * look at a single program.  Every value is its own raw DEFLATE stream (RFC
 * 1951), so a corpus is as many independent decoders as it has records.  The
 * write side (Save, Delete, Flush and compact: "the corpus database, written"
 * below) has its compressor in csrc/sg_deflate.h.
 *
 * The decoder (csrc/sg_inflate.h, one source for host and device) follows
 * zlib 1.2.11's inflate of a raw stream.  A stream's status:
 *   SG_INFLATE_OK 0 the final block ended; SG_INFLATE_CORRUPT 1 zlib raises;
 *   SG_INFLATE_TRUNCATED 2 the input ended before the final block did, and
 *   nothing corrupt was seen before that point; SG_INFLATE_TOO_LARGE 3 the
 *   output reached 2^32 bytes (this library's limit per stream, not zlib's:
 *   the decoder stops there; reached by a CPU test of the decoder only, no
 *   GPU test inflates 4 GiB).
 * consumed is the number of input bytes up to and including the byte that
 * holds the last bit of the final block (0 unless OK); bytes after it are
 * ignored, as Go's reader ignores them inside the LimitedReader of :242.
 * A stream as Go writes it (Flush then Close of a flate.Writer, :161-162) is
 * read here, from that package's source, as the deflate data, an empty stored
 * block (sync flush) and the final empty stored block 01 00 00 ff ff; the
 * source is not part of this repository's references, so parity with Go's
 * writer is unpinned -- any valid stream is decoded whatever wrote it.
 * A stream longer than SG_INFLATE_LONG compressed bytes gets a wave to itself;
 * the context counter "inflate_long_streams" counts them, "inflate_long_len"
 * is the constant. */
#define SG_INFLATE_OK 0
#define SG_INFLATE_CORRUPT 1
#define SG_INFLATE_TRUNCATED 2
#define SG_INFLATE_TOO_LARGE 3
#define SG_INFLATE_LONG 65536
/* A CSR of streams in, a CSR of outputs out: stream k is in[in_off[k] ..
 * in_off[k+1]) and owns out[out_off[k] .. out_off[k+1]); a stream that is not
 * OK owns no output.  status, consumed (n each) and out_off (n + 1) are always
 * written; *nout is always the total, and out is written only when it is <=
 * cap.  SG_EINVAL, before the context is touched: a NULL ctx, out_off or nout;
 * status or consumed NULL with n > 0; out NULL with cap > 0; what
 * sg_prog_hashes rejects of a CSR; 2^32 streams or more.  SG_EINVAL after the
 * count pass, with nothing written: 2^33 output bytes or more.  SG_ENODEV
 * without a device.  Two waits. */
int sg_inflate_batch(sg_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t n, uint8_t* status,
		     uint64_t* consumed, uint64_t* out_off, uint8_t* out, size_t cap, size_t* nout);
/* Device form (nbytes = the bytes in d_in): every pointer is device memory,
 * stream-ordered, nothing is read back; d_out_off[n] is the total and d_out is
 * written only when it is <= cap.  The offsets follow sg_prog_hashes_dev's
 * rule: each start is clamped to nbytes and each end to [start, nbytes], so
 * garbage offsets give garbage streams (which mostly fail), never a read
 * outside [d_in, d_in + nbytes) or a write outside [d_out, d_out + cap).
 * SG_EINVAL: a NULL ctx or d_out_off; d_in_off, d_status or d_consumed NULL
 * with n > 0; d_in NULL with nbytes > 0; d_out NULL with cap > 0; n >= 2^32. */
int sg_inflate_batch_dev(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, uint64_t n, uint64_t nbytes,
			 uint8_t* d_status, uint64_t* d_consumed, uint64_t* d_out_off, uint8_t* d_out, uint64_t cap);

/* deserializeHeader (:193-211) and the framing half of deserializeRecord
 * (:213-249) over a file's bytes; host only: no context, no device.  Records
 * come in file order: key = bytes[key_pos .. + key_len), seq, and the value's
 * stream bytes[val_pos .. + val_len).  seq == ~0 is a deletion and has no
 * value field (val_pos = val_len = 0); val_len == 0 is an empty value.  *end:
 *   SG_DB_END_EOF 0 clean end at a record boundary; SG_DB_END_MAGIC 1 bad
 *   header magic; SG_DB_END_VERSION 2 bad version (0, or above 1);
 *   SG_DB_END_RECORD 3 bad record magic; SG_DB_END_TRUNCATED 4 a header field,
 *   a key or a value runs past the file.
 * The record at which *end != 0 arises is not counted.  An empty file is a
 * valid empty database (:196-198); a file of 1 to 7 bytes is end 4, or end 1
 * once four bytes disagree with the magic.  A record's framing always advances
 * by val_len, whatever the stream inside consumed: the reference leaves that
 * to how far its inner bufio reader happened to read, so this is a pinned
 * choice and parity is unpinned where a stream ends before its frame.
 * *nrec is always the count; the arrays are written only when it is <= cap.
 * SG_EINVAL: a NULL nrec or end, bytes NULL with nbytes > 0, an array NULL
 * with cap > 0.  The return value is SG_OK whatever *end is. */
#define SG_DB_END_EOF 0
#define SG_DB_END_MAGIC 1
#define SG_DB_END_VERSION 2
#define SG_DB_END_RECORD 3
#define SG_DB_END_TRUNCATED 4
#define SG_DB_END_VALUE 5
#define SG_DB_SEQ_DELETED (~0ull)
int sg_db_scan(const uint8_t* bytes, size_t nbytes, uint64_t* key_pos, uint32_t* key_len, uint64_t* seq,
	       uint64_t* val_pos, uint32_t* val_len, size_t cap, size_t* nrec, int* end);

/* db.Open (:38-52) without the compaction: the file is scanned on the host
 * and uploaded once, and EVERY framed stream is counted and validated on the
 * device.  The first record whose stream is not OK ends the database there,
 * as deserializeDB :180-183 returns at the first error -- also when a later
 * record would have overwritten it -- and end becomes SG_DB_END_VALUE 5.  Over
 * the prefix that parsed, the last write of a key wins and a deletion removes
 * the key (:185-189), resolved on the host after the one read-back of statuses
 * and lengths; only the live records' streams are then written out.  Live
 * records are in file order of their winning write: Go has map order there, so
 * this is a pinned choice, not a parity claim.  The texts stay on the device
 * until sg_db_destroy.  SG_EINVAL: a NULL ctx or out, bytes NULL with nbytes >
 * 0; 2^32 records or 2^33 text bytes or more.  SG_ENODEV without a device.
 * The database lives in ctx and must be destroyed before it. */
typedef struct sg_db sg_db;
int sg_db_open(sg_ctx* ctx, const uint8_t* bytes, size_t nbytes, sg_db** out);
void sg_db_destroy(sg_db* db);
/* counts[0] nlive = len(db.Records); [1] uncompacted, the records parsed,
 * deletions included (:184); [2] the live texts' bytes; [3] the live keys'
 * bytes; [4] end. */
int sg_db_counts(sg_db* db, uint64_t counts[5]);
/* The live records to the host: key_off (nlive + 1) and keys, seqs (nlive),
 * text_off (nlive + 1) and texts, sized by sg_db_counts; any of them may be
 * NULL.  One wait when texts or text_off are asked for. */
int sg_db_export(sg_db* db, uint64_t* key_off, uint8_t* keys, uint64_t* seqs, uint64_t* text_off, uint8_t* texts);
/* The device pointers of the texts and their nlive + 1 offsets, as
 * sg_prog_hashes_dev and sg_call_sets_dev take them; valid until
 * sg_db_destroy. */
int sg_db_device(sg_db* db, const uint8_t** d_texts, const uint64_t** d_text_off);
/* loadDB's loop (state.go:91-105) over the resident texts; no text crosses the
 * bus again.  bad[k] = 1 when prog.CallSet fails (sg_call_sets_dev's status is
 * not 0), else 2 when the key is not exactly the 40 lower-case hex characters
 * of sg_prog_hashes_dev's hash, else 0; *max_seq is taken over the records
 * with bad == 0 (:102-104).  tab may be NULL (no ids are looked up); one of
 * another context is SG_EINVAL, as are a NULL db or max_seq and bad NULL with
 * live records.  One wait. */
int sg_db_verify(sg_db* db, sg_nametab* tab, uint8_t* bad, uint64_t* max_seq);

/* ---- the corpus database, written: deflate, serializeRecord and compact ------ */
/* pkg/db's write side: serializeRecord (pkg/db/db.go:137-165) deflates a value
 * at flate.BestCompression, on one thread; compact() (:95-116) does that to
 * every live record, and Flush (:75-93) reaches it from minimizeCorpus under
 * mgr.mu (syz-manager/manager.go:786-795), from the end of the hub's loadDB
 * (syz-hub/state/state.go:106) and from purgeCorpus (:349-351); Open reaches it
 * when nine tenths of the file is dead (:48-50); the hub's addInputs
 * (state.go:310-336) is a run of Saves and two Flushes.
 *
 * The encoder (csrc/sg_deflate.h, one source for host and device) writes a
 * value as ONE block, fixed or dynamic, or as a chain of stored blocks of at
 * most 65,535 bytes, whichever is shortest in bytes (of equal lengths: stored
 * before fixed before dynamic); the last block carries BFINAL and nothing
 * follows it.  The empty input is 03 00.  The parse is LZ77 with a 512-entry
 * table of last positions, greedy, one probe; the dynamic code's lengths are
 * Shannon lengths made complete, not Huffman's.  Go's reader takes any valid
 * stream inside its LimitedReader (:242); equality with the bytes Go's
 * flate.Writer would have written is no goal, and parity with it stays
 * unpinned as said above.  A stream's bytes depend on its input bytes alone:
 * not on the batch, not on the side that ran it.
 * An input longer than SG_DEFLATE_LONG bytes gets a wave to itself; the context
 * counter "deflate_long_streams" counts them, "deflate_long_len" is the
 * constant. */
#define SG_DEFLATE_LONG 65536
/* The stored form's length, len + 5 * max(1, ceil(len / 65535)): what no
 * stream of len input bytes exceeds.  Host only. */
size_t sg_deflate_bound(size_t len);
/* The encoder on the host: no device, no context (as sg_db_scan has none), for
 * a lone Save (manager.go:921-922) whose bytes are then what the device would
 * have written.  A CSR of inputs in, a CSR of streams out: out_off (n + 1) is
 * always written, *nout is always the total, and out is written only when it
 * is <= cap (out NULL with cap 0 is the count form).  SG_EINVAL: a NULL out_off
 * or nout; out NULL with cap > 0; what sg_prog_hashes rejects of a CSR; an
 * input of more than 2^32 - 2^20 bytes. */
int sg_deflate_host(const uint8_t* in, const uint64_t* in_off, size_t n, uint64_t* out_off, uint8_t* out, size_t cap,
		    size_t* nout);
/* The same on the device, a lane per stream, with sg_inflate_batch's
 * conventions.  SG_EINVAL, before the context is touched: a NULL ctx, and what
 * sg_deflate_host rejects.  SG_EINVAL after the count phase, with nothing
 * written: 2^33 output bytes or more.  SG_ENODEV without a device.  Two waits. */
int sg_deflate_batch(sg_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t n, uint64_t* out_off, uint8_t* out,
		     size_t cap, size_t* nout);
/* Device form (nbytes = the bytes in d_in): every pointer is device memory,
 * stream-ordered, nothing is read back; d_out_off[n] is the total and d_out is
 * written only when it is <= cap.  Offsets are clamped as sg_inflate_batch_dev
 * clamps them; an input is cut at 2^32 - 2^20 bytes.  SG_EINVAL: a NULL ctx or
 * d_out_off; d_in_off NULL with n > 0; d_in NULL with nbytes > 0; d_out NULL
 * with cap > 0; n >= 2^32. */
int sg_deflate_batch_dev(sg_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, uint64_t n, uint64_t nbytes,
			 uint64_t* d_out_off, uint8_t* d_out, uint64_t cap);
/* serializeHeader (when with_header != 0) and serializeRecord (:132-165) for n
 * records in the given order: record k has key keys[key_off[k] ..
 * key_off[k+1]), seq seqs[k] and value texts[text_off[k] .. text_off[k+1]).
 * Each record is the magic 0xfee1bad, u32 len(key), the key and u64 seq; for
 * seq == SG_DB_SEQ_DELETED it ends there; otherwise u32 val_len and the stream
 * follow, and an empty value has val_len 0 and no stream (:148-149).  The
 * whole byte string is assembled on the device and downloaded once.  *nout is
 * always its length; out is written only when it is <= cap.  SG_EINVAL, before
 * the context is touched: a NULL ctx or nout; seqs NULL with n > 0; out NULL
 * with cap > 0; what sg_prog_hashes rejects of either CSR; a key of 2^32 bytes
 * or more; a deletion with a non-empty value (Go panics, :143-145); a value
 * whose stream could reach 2^32 bytes (more than 2^32 - 2^20 bytes of input).
 * SG_EINVAL after the count phase: a file of 2^33 bytes or more.  SG_ENODEV
 * without a device.  Two waits. */
int sg_db_serialize(sg_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, const uint64_t* seqs, const uint8_t* texts,
		    const uint64_t* text_off, size_t n, int with_header, uint8_t* out, size_t cap, size_t* nout);
/* compact()'s buffer (:96-100) for an opened database, from its resident texts
 * with no upload but the keys: the header, then the live records in
 * sg_db_export's order (Go has map order there; the pinned choice of
 * sg_db_open).  *nout and out as above.  SG_EINVAL: a NULL db or nout, out NULL
 * with cap > 0. */
int sg_db_compact(sg_db* db, uint8_t* out, size_t cap, size_t* nout);

/* ---- cover report ingest: binutils text to the cover table's arrays ---------- */
/* What stands between vmlinux and sg_cover_table_create: the reference scans
 * all of `objdump -d --no-show-raw-insn vmlinux` for the __sanitizer_cov_trace_pc
 * call sites (coveredPCs, syz-manager/cover.go:310-347) and sorts them
 * (initAllCover, :64-89), and parses `nm -nS vmlinux` (symbolizer.ReadSymbols,
 * pkg/symbolizer/nm.go:19-69) into the symbols that uncoveredPcsInFuncs
 * flattens and sorts (cover.go:262-268).  Both are byte-parallel scans of a
 * text; here each is one call over the whole text.
 *
 * Lines, pinned (bufio.Scanner / ScanLines, as for prog.CallSet above): the
 * text is split at '\n'; the bytes after the last '\n' are a line only if there
 * are any; one trailing '\r' is dropped from each line; empty lines are lines.
 * The scanner's limit is bufio.MaxScanTokenSize: a line whose content -- the
 * bytes before its '\n' or before the end of the text, the '\r' counted -- is
 * SG_INGEST_MAX_LINE bytes or more makes the whole call fail as the
 * reference's s.Err() does: status SG_INGEST_TOO_LONG, err_pos the byte offset
 * of the first such line's start, a count of 0 and no other output.  That
 * boundary is read, not run (Go is not needed to build or test this library).
 *
 * A hex field is strconv.ParseUint(field, 16, 64): at least one byte, every
 * byte in [0-9a-fA-F] (no sign, no "0x", no '_', no blank), the value at most
 * 2^64 - 1 -- judged by value, so any number of leading zeros is fine and a
 * seventeenth significant digit is an error. */
#define SG_INGEST_OK 0
#define SG_INGEST_TOO_LONG 1
#define SG_INGEST_MAX_LINE 65536
#define SG_INGEST_MAX_NEEDLE 64

/* coveredPCs (cover.go:310-347) and the sort of cover.go:78.  Of each line:
 * pos is the first occurrence of `call` (call_len bytes); `func` must occur in
 * ln[pos:] (it may overlap the call match); colon is the first ':' of the
 * line; ln[:colon] must be a hex field as above (so a line that objdump
 * indents with blanks is skipped).  A line that fails any step is skipped
 * silently.  The reference's needles are "callq " and
 * " <__sanitizer_cov_trace_pc>"; newer binutils print "call ".  pcs receives the
 * PCs ascending, duplicates kept; *npcs is always their number and pcs is
 * written only when it is <= cap.  nbytes / 2 + 1 always suffices as cap (a
 * kept line is at least a digit and ':'; the needles may overlap the field).  SG_EINVAL, before the context is touched: a NULL
 * ctx, npcs, status or err_pos; text NULL with nbytes > 0; pcs NULL with cap >
 * 0; a NULL needle or a needle length outside 1..SG_INGEST_MAX_NEEDLE; 2^33
 * bytes of text or more.  SG_ENODEV without a device.  Two waits (the count,
 * the PCs), and one more inside the sort. */
int sg_objdump_pcs(sg_ctx* ctx, const uint8_t* text, size_t nbytes, const uint8_t* call, size_t call_len,
		   const uint8_t* func, size_t func_len, uint64_t* pcs, size_t cap, size_t* npcs, uint32_t* status,
		   uint64_t* err_pos);
/* Device form: d_text and d_pcs are device memory (the needles stay host
 * memory), and the PCs stay resident; d_info (device, 3 words) receives
 * {count, status, err_pos}.  The call waits once for the count, which sizes
 * the sort; nothing else is read back. */
int sg_objdump_pcs_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, const uint8_t* call, size_t call_len,
		       const uint8_t* func, size_t func_len, uint64_t* d_pcs, uint64_t cap, uint64_t* d_info);

/* symbolizer.ReadSymbols (nm.go:19-69) and the flatten-and-sort of
 * cover.go:262-268.  Of each line: sp1 is the first ' ', sp2 the next ' '
 * after it; ln[sp2:] must start with " t " or " T " (which is also the
 * reference's first test, that the line contains one of the two); ln[:sp1]
 * and ln[sp1+1:sp2] must be hex fields as above, addr and size; name =
 * ln[sp2+3:], which may be empty and may contain blanks.  A line that fails any
 * step is skipped, so `0000000000401000 T _init` (no size column) is.
 * Size = int(size+15)/16*16: the add wraps in 64 bits, the sum is taken as
 * int64, the division truncates toward zero; end = addr + uint64(Size), wrapping.
 *
 * Symbol k, in text order: addr[k], size[k] (Size), and its name's bytes
 * text[name_pos[k] .. name_pos[k] + name_len[k]).  sym_start / sym_end are the
 * symbols in the order sg_cover_uncovered and sg_cover_table_create want,
 * ascending by start, and order[j] is the text-order index of the symbol in
 * sorted place j.  The reference flattens a map and sorts with the unstable
 * sort.Sort, so its order among equal starts is undefined; here it is pinned
 * as (start, text order).  Any of the seven arrays may be NULL (not wanted).
 * *nsyms is always the number of symbols; the arrays are written only when
 * it is <= cap.  nbytes / 6 + 1 always suffices as cap.  SG_EINVAL, before the
 * context is touched: a NULL ctx, nsyms, status or err_pos; text NULL with
 * nbytes > 0; 2^33 bytes of text or more.  SG_EINVAL after the count: 2^32 - 1
 * symbols or more.  SG_ENODEV without a device.  Two waits. */
int sg_nm_symbols(sg_ctx* ctx, const uint8_t* text, size_t nbytes, uint64_t* addr, int64_t* size, uint64_t* name_pos,
		  uint32_t* name_len, uint64_t* sym_start, uint64_t* sym_end, uint32_t* order, size_t cap, size_t* nsyms,
		  uint32_t* status, uint64_t* err_pos);
/* Device form: every array is device memory, d_info as sg_objdump_pcs_dev's;
 * one wait, for the count. */
int sg_nm_symbols_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, uint64_t* d_addr, int64_t* d_size,
		      uint64_t* d_name_pos, uint32_t* d_name_len, uint64_t* d_sym_start, uint64_t* d_sym_end,
		      uint32_t* d_order, uint64_t cap, uint64_t* d_info);

/* symbolize and parse (pkg/symbolizer/symbolizer.go:95-191) over the whole
 * output of `addr2line -afi` for nrec PCs (the reference's len(pcs): the record
 * of its sentinel 0xffffffffffffffff, and anything behind the start of record
 * nrec, is never looked at), with the interning that fileSet's string compares
 * need (sg_cover_table_create: "equal strings MUST get equal ids").
 *
 * Lines as above.  The first line is record 0's PC line.  After it a record
 * starts at a line with len > 3, ln[0] == '0' and ln[1] == 'x' met where a
 * function line is expected; function and file lines alternate.  A PC line is
 * strconv.ParseUint(line, 0, 64): "0x" / "0X" hex, "0b" binary, "0o" or a
 * leading "0" octal, else decimal, '_' between digits as base 0 allows.  Of a
 * file line colon is the LAST ':', the line number the digits that follow it
 * (so ":588 (discriminator 3)" is 588) and file = ln[:colon].  A frame is
 * dropped, its two lines consumed, when the digits are empty or overflow int
 * (64 bits), fn or file is "" or "??", or line <= 0.  A record may have no
 * frames.  The last record ends at the next start, at a "0x" line with a ':'
 * where a function line is expected (the reference leaves parse there and never
 * parses again), or at the end of the text.
 *
 * The whole call fails (status, and err_pos the byte offset of the failing
 * line's start; the first failure in text order, no other output) on:
 *   SG_A2L_EMPTY 1         no line at all (err_pos 0);
 *   SG_A2L_BAD_PC 2        a PC line that does not parse -- the first line, or
 *                          a "0x" line with a ':' where a function line is
 *                          expected before the last record;
 *   SG_A2L_NO_COLON 3      a file line without ':' (a record start met where a
 *                          file line is expected is one);
 *   SG_A2L_NO_FILE_LINE 4  the text ends behind a function line (err_pos: that
 *                          line);
 *   SG_A2L_TOO_LONG 5      a line of SG_INGEST_MAX_LINE bytes or more among the
 *                          lines read;
 *   SG_A2L_TOO_FEW 6       fewer than nrec records (err_pos nbytes; the
 *                          reference would block on its pipe).
 * The records are found in parallel: after line 0 the starts are the "0x"
 * lines without ':' (in a text the reference parses, exactly those), a scan
 * gives each line its record and its place in it, and place parity and shape
 * turn into the failures above.
 *
 * rec_pc[r] is record r's PC; its kept frames are frame_off[r] ..
 * frame_off[r+1] (nrec + 1 entries) of frame_file / frame_line / frame_func,
 * in text order.  File and Func ids are dense in order of first occurrence
 * among the kept frames, which is what setdefault(name, len(dict)) gives; id
 * k's bytes are text[file_pos[k] .. + file_len[k]) (func_pos / func_len
 * likewise), its first occurrence.  Names are hashed (FNV-1a, 64 bits; hash_bits,
 * 1..64, 64 in production, masks the first round's hash so a test can force
 * the path below: the results are the same at every value) and grouped by hash, and every member of a group is
 * compared with the group's first BY BYTES; when any group holds two different
 * names the whole column is grouped again under another seed of the full hash
 * (at most 4 rounds, then SG_EHIP: never a wrong id, never a host fallback).
 * info (6 words): {frames, nfiles, nfuncs, status, err_pos, extra rounds}.
 * The frame and name arrays are written only when frames <= cap (names never
 * outnumber frames).  SG_EINVAL, before the context is touched: a NULL ctx or
 * info; text NULL with nbytes > 0; rec_pc or frame_off NULL; a frame or name
 * array NULL with cap > 0; nrec >= 2^32 - 1; hash_bits outside 1..64; 2^33
 * bytes of text or more.
 * SG_EINVAL after the line count: 2^32 - 1 lines or more.  SG_ENODEV without a
 * device.  A wait each for the line count, the frame count and every interning
 * round. */
#define SG_A2L_OK 0
#define SG_A2L_EMPTY 1
#define SG_A2L_BAD_PC 2
#define SG_A2L_NO_COLON 3
#define SG_A2L_NO_FILE_LINE 4
#define SG_A2L_TOO_LONG 5
#define SG_A2L_TOO_FEW 6
int sg_addr2line_frames(sg_ctx* ctx, const uint8_t* text, size_t nbytes, size_t nrec, uint64_t* rec_pc,
			uint64_t* frame_off, uint32_t* frame_file, int64_t* frame_line, uint32_t* frame_func, size_t cap,
			uint64_t* file_pos, uint32_t* file_len, uint64_t* func_pos, uint32_t* func_len, uint32_t hash_bits,
			uint64_t* info);
/* Device form: every array and info are device memory; the same waits. */
int sg_addr2line_frames_dev(sg_ctx* ctx, const uint8_t* d_text, uint64_t nbytes, uint64_t nrec, uint64_t* d_rec_pc,
			    uint64_t* d_frame_off, uint32_t* d_frame_file, int64_t* d_frame_line, uint32_t* d_frame_func,
			    uint64_t cap, uint64_t* d_file_pos, uint32_t* d_file_len, uint64_t* d_func_pos,
			    uint32_t* d_func_len, uint32_t hash_bits, uint64_t* d_info);

/* The cover table straight from the tools' text: sg_nm_symbols over nm_text,
 * sg_addr2line_frames over a2l_text for nrec records, and the table that
 * sg_cover_table_create would build from their arrays with tab_pcs = the
 * records' PCs -- indistinguishable from it through sg_cover_lines and
 * sg_cover_pages.  The records' PCs, frame_off and the frame arrays are never on
 * the host: they go from the parse to the table on the device.  The symbols
 * (a few MB of text) and all_pcs, the call sites (host memory; sg_objdump_pcs'
 * result, which must be distinct), are host arrays, as the table's plan reads
 * them there.  What sg_cover_table_create demands of the rest is checked on the
 * device and reported as SG_EINVAL after the build's wait, with no table: the
 * records' PCs strictly ascending, every call site among them, every line
 * below 2^32.  The names come back as sg_addr2line_frames returns them, when
 * the frames (which names never outnumber) are <= names_cap; with more, only
 * the counts come back, *out stays NULL and the call is made again.
 * info (8 words): sg_addr2line_frames' six, then sg_nm_symbols' status and
 * err_pos; with either status set *out stays NULL and the call returns SG_OK.
 * SG_EINVAL, before the context is touched: a NULL ctx, out or info; a text
 * NULL with bytes; all_pcs NULL with nall > 0; a name array NULL with
 * names_cap > 0; nrec >= 2^32 - 1; hash_bits outside 1..64; a text of 2^33
 * bytes or more.  SG_EINVAL later: symbols or call sites out of order
 * (host), 2^32 - 1 frames or more.  SG_ENODEV without a device.  The table
 * belongs to ctx (sg_cover_lines rejects a set of another context as before). */
int sg_cover_table_from_text(sg_ctx* ctx, const uint8_t* nm_text, size_t nm_bytes, const uint64_t* all_pcs, size_t nall,
			     const uint8_t* a2l_text, size_t a2l_bytes, size_t nrec, uint32_t hash_bits, uint64_t* file_pos,
			     uint32_t* file_len, uint64_t* func_pos, uint32_t* func_len, size_t names_cap, uint64_t* info,
			     sg_cover_table** out);

/* ---- pkg/report over a batch of console logs ---------------------------
 * report.ContainsCrash (pkg/report/report.go:369-387), report.Parse up to
 * extractDescription (:393-465) and report.ExtractConsoleOutput (:492-513)
 * walk a log line by line and run, for every line, the header searches of
 * matchOops (:515-531) and two regular expressions (:348-349).  Here each is
 * one call over a batch of logs -- a crash store's log files -- as a CSR:
 * `bytes`, off[nlogs + 1].  Positions are uint64 and relative to their log's
 * start unless said otherwise.
 *
 * Lines, pinned (the loop of :370-376, not bufio.Scanner): a log is split at
 * '\n'; the bytes after the last '\n' are a line only if there are any; empty
 * lines are lines; '\r' stays part of the line; a line has no length limit;
 * nothing matches across the end of a log into the next one.
 *
 * The oops table (:29-345) is fixed in the library, SG_CRASH_OOPSES headers in
 * the reference's order: 0 "BUG:", 1 "WARNING:", 2 "INFO:", 3 "Unable to handle
 * kernel paging request", 4 "general protection fault:", 5 "Kernel panic",
 * 6 "kernel BUG", 7 "Kernel BUG", 8 "BUG kmalloc-", 9 "divide error:",
 * 10 "invalid opcode:", 11 "unreferenced object", 12 "UBSAN:".  A line matches
 * oops i when it contains header i -- `match` is the leftmost occurrence's
 * offset in the line -- and no suppression of oops i matches anywhere in the
 * line: "Boot_DEBUG:" for 0; "WARNING: /etc/ssh/moduli does not exist, using
 * fixed modulus" for 1; "INFO: lockdep is turned off", "INFO: Stall ended
 * before state dump start", "_INFO::" and `INFO: NMI handler .* took too long
 * to run` for 2, the last holding exactly when some " took too long to run"
 * starts at or behind the end of the leftmost "INFO: NMI handler ".  A
 * suppression removes only its own oops.
 *
 * A console line is one where `^(?:<[0-9]+>)?\[ *[0-9]+\.[0-9]+\] ` matches at
 * the start and which holds no match of ` \? +[a-zA-Z0-9_.]+\+0x[0-9a-f]+/
 * [0-9a-f]+` or holds "<EOI>".  Its body runs from the end of that prefix to
 * the line's end, less one trailing '\r'.
 *
 * Geometry the tests are cut to: the kernels read the batch in tiles of
 * SG_CRASH_TILE bytes, each with the SG_CRASH_MAX_LITERAL - 1 bytes behind it;
 * SG_CRASH_MAX_LITERAL is the longest literal (the sshd sentence).  stats
 * (nullable, SG_CRASH_NSTATS words): {lines, console lines (sg_crash_parse),
 * records (sg_crash_scan)} of the call, 0 where the call does not count it. */
#define SG_CRASH_OOPSES 13
#define SG_CRASH_TILE 4096
#define SG_CRASH_MAX_LITERAL 60
#define SG_CRASH_NSTATS 3

/* The header search.  One record per (line, matching oops), ordered by (log,
 * line, table order): rec_log, the line's start and end (the '\n' position or
 * the log's length), rec_oops and rec_match.  contains[l] = 1 where log l has
 * a record: ContainsCrash without ignores.  *nrec is always the number of
 * records; the five arrays are written only when it is <= cap.  The batch's
 * bytes always suffice as cap.  The caller's `ignores` depend on the line
 * alone: it runs them over the few lines that have records and hands the
 * ignored lines to sg_crash_parse.  SG_EINVAL, before the context is touched:
 * a NULL ctx or nrec; contains NULL with nlogs > 0; a record array NULL with
 * cap > 0; what sg_prog_hashes rejects of the CSR; 2^32 bytes or more.
 * SG_ENODEV without a device.  Two waits (the line count, the record count)
 * and a third for the records. */
int sg_crash_scan(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, uint8_t* contains,
		  uint32_t* rec_log, uint64_t* rec_start, uint64_t* rec_end, uint32_t* rec_oops, uint64_t* rec_match,
		  size_t cap, size_t* nrec, uint64_t* stats);
/* Device form: every pointer is device memory, stream-ordered; *d_nrec is the
 * count.  One wait, for the line count, which sizes the workspace.  The
 * offsets follow sg_prog_hashes_dev's rule (clamped to nbytes; garbage gives
 * garbage, never a read outside [d_bytes, d_bytes + nbytes)), and the batch
 * ends at min(d_off[nlogs], nbytes). */
int sg_crash_scan_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
		      uint8_t* d_contains, uint32_t* d_rec_log, uint64_t* d_rec_start, uint64_t* d_rec_end,
		      uint32_t* d_rec_oops, uint64_t* d_rec_match, uint64_t cap, uint64_t* d_nrec, uint64_t* d_stats);

/* Everything of Parse before extractDescription.  ign_off[nlogs + 1], ign_pos
 * (NULL ign_off: none): the starts of the lines the caller's ignores match,
 * ascending per log; a record whose line is listed does not exist.  Per log:
 * oops (-1: none; then the other four are 0 and the log has no text), start =
 * the start of the first line with a record, end = the end of the last such
 * line, desc_pos / desc_len = output[pos + match : next] of the first line for
 * its first oops in table order, which is also extractDescription's fallback
 * (:554-564).  text_off[nlogs + 1] / text: the report text of :417-459.  With
 * L0 the first line with a record: nothing when no console line stands at or
 * after L0; else the bodies, each followed by '\n', of the last five console
 * lines before L0, then of the console lines from L0 on that do not contain
 * "Disabling lock debugging due to kernel taint", all of it up to but
 * excluding the cut: the first console line at or after L0 whose rank among
 * those is above 40, which contains "Kernel panic - not syncing" and not the
 * taint sentence.  *ntext is always the text's bytes; text is written only
 * when it is <= cap.  The batch's bytes always suffice as cap.  SG_EINVAL,
 * before the context is touched: a NULL ctx, text_off or ntext; a per-log
 * array NULL with nlogs > 0; text NULL with cap > 0; what sg_crash_scan
 * rejects of the CSR; ignore offsets that are no CSR's, or places that do not
 * ascend or lie outside their log.  SG_ENODEV without a device.  Three waits. */
int sg_crash_parse(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, const uint64_t* ign_off,
		   const uint64_t* ign_pos, int32_t* oops, uint64_t* start, uint64_t* end, uint64_t* desc_pos,
		   uint64_t* desc_len, uint64_t* text_off, uint8_t* text, size_t cap, size_t* ntext, uint64_t* stats);
/* Device form, as sg_crash_scan_dev's: d_text_off[nlogs] is the total and
 * d_text is written only when it is <= cap (compared on the device); the
 * ignore list's nign places are device memory too, its offsets clamped. */
int sg_crash_parse_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
		       const uint64_t* d_ign_off, const uint64_t* d_ign_pos, uint64_t nign, int32_t* d_oops,
		       uint64_t* d_start, uint64_t* d_end, uint64_t* d_desc_pos, uint64_t* d_desc_len,
		       uint64_t* d_text_off, uint8_t* d_text, uint64_t cap, uint64_t* d_stats);

/* ExtractConsoleOutput: every console line's body and a '\n', per log.
 * Counts, cap and SG_EINVAL as sg_crash_parse's. */
int sg_console_output(sg_ctx* ctx, const uint8_t* bytes, const uint64_t* off, size_t nlogs, uint64_t* out_off,
		      uint8_t* out, size_t cap, size_t* nout, uint64_t* stats);
int sg_console_output_dev(sg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t nlogs, uint64_t nbytes,
			  uint64_t* d_out_off, uint8_t* d_out, uint64_t cap, uint64_t* d_stats);

#ifdef __cplusplus
}
#endif

#endif /* SYZSIG_H */
