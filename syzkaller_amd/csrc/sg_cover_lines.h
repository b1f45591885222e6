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
