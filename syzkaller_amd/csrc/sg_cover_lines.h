// sg_cover_lines.h -- the report table and the line-table stage of
// sg_cover_lines.hip, for what renders from its results while they are still
// on the device (sg_cover_pages.hip).
#pragma once

#include "sg_report.h"

struct sg_cover_table {
  sg_ctx* ctx = nullptr;
  sg::DevBuf<char> mem;  // the one device block everything below lives in
  bool has_rep = false;  // symbols and call sites: the uncovered side exists
  sg::RepTables rep{};
  uint64_t nsym = 0, nall = 0, ntab = 0, nfr = 0, nslots = 0;
  uint32_t nfiles = 0, nfuncs = 0;
  uint64_t* tab = nullptr;  // [ntab]
  sg::RadixIdx itab{};
  uint32_t* site_row = nullptr;       // [nall] each call site's row of tab
  uint32_t* frame_off = nullptr;      // [ntab + 1]
  uint32_t* frame_slot = nullptr;     // [nfr]
  uint32_t* frame_func = nullptr;     // [nfr]
  uint32_t* frame_file = nullptr;     // [nfr]
  uint32_t* slot_line = nullptr;      // [nslots]
  uint32_t* file_slot_off = nullptr;  // [nfiles + 1]
};

namespace sg {

// Where a table's PCs and frames come from.  Host arrays, checked by sg_cover_table_create; or, with dev, device
// arrays that lie in the context's workspace below dev->ws_base (sg_cover_ingest.hip leaves them there), checked on
// the device.  vary: the bits in which the frames' file << 32 | line keys differ (0: all equal).
struct CoverTableDev {
  const uint64_t* tab;        // [ntab]
  const uint64_t* frame_off;  // [ntab + 1]
  const uint32_t* frame_file;
  const int64_t* frame_line;
  const uint32_t* frame_func;
  size_t ws_base;
};
struct TableSrc {
  const uint64_t* tab_pcs;
  const uint64_t* frame_off;
  const uint32_t *frame_file, *frame_line, *frame_func;
  const CoverTableDev* dev;
  uint64_t vary;
};
// (ctx lock held, the device ensured; the symbols and call sites are host arrays that sg_cover_table_create's rules
// hold for.)  The workspace must hold ws_base + cover_table_build_ws(nfr) bytes already when src.dev is set: the
// build does not move it.
int table_build(sg_ctx* ctx, const char* fn, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym,
                const uint64_t* all_pcs, size_t nall, size_t ntab, uint64_t tab_lo, uint64_t tab_hi, uint64_t nfr,
                uint32_t nfiles, uint32_t nfuncs, const TableSrc& src, sg_cover_table** out);
size_t cover_table_build_ws(uint64_t nfr);
// what sg_cover_table_create asks of the symbols and the call sites (host arrays)
int table_syms_ok(const char* fn, const uint64_t* sym_start, const uint64_t* sym_end, size_t nsym, const uint64_t* all_pcs,
                  size_t nall);

// A report's line tables as cover_lines_body leaves them in the workspace:
// file f's lines are lines[file_off[f] .. file_off[f + 1]), ascending, cov
// alongside; only file_off[nfiles] <= nslots entries are written.
struct LinesDev {
  const uint64_t* file_off;  // [nfiles + 1]
  const uint32_t* lines;     // [nslots]
  const uint8_t* cov;        // [nslots]
};

// What a caller hangs on a report.  ws_bytes of the workspace are reserved
// for it behind the report's own, at the offset `queued` is told.  queued
// runs when every kernel of the report is on the stream, before the wait for
// its counts: what it launches and copies to the host is covered by that wait.
// counted runs after the wait, before the results are fetched: what it queues
// then is covered by the wait for them, which is made whenever *more is set.
// Neither may reserve the workspace.
struct LinesTail {
  size_t ws_bytes = 0;
  virtual int queued(const LinesDev& d, size_t ws_off) = 0;
  virtual int counted(bool* more) = 0;

 protected:
  ~LinesTail() = default;
};

// Both report forms behind their argument checks (ctx lock held, the device
// ensured): d_cov is device memory of the context (its staging buffer).
int cover_lines_body(sg_cover_table* t, const uint32_t* d_cov, uint64_t ncov, uint32_t base, uint64_t* file_off,
                     uint32_t* lines, uint8_t* covered, uint8_t* file_seen, uint64_t* ncovered_frames,
                     uint64_t* missing, size_t* nmissing, LinesTail* tail = nullptr);
// the checks and the empty result the two host forms share
int lines_args_ok(const char* fn, sg_cover_table* t, uint64_t* file_off, uint32_t* lines, uint8_t* covered,
                  uint64_t* ncovered_frames, uint64_t* missing, size_t* nmissing);
void lines_empty(sg_cover_table* t, uint64_t* file_off, uint8_t* file_seen, uint64_t* ncovered_frames,
                 size_t* nmissing);
// The cover of the set form, ascending, in the context's staging buffer at
// offset 0 (nothing uploaded; ctx lock held, the device ensured).
int lines_set_cover(const char* fn, sg_ctx* ctx, sg_set* cov, uint64_t* total);

}  // namespace sg
