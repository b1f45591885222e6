// sg_rank.h -- distinct values and ranks of u64 keys through the radix sort,
// and the driver of the calls that have a fast shape and a general path
// (sg_rank.hip).  Its users: sg_exec_comps.hip, sg_exec_cover.hip,
// sg_hints.hip, sg_cover_lines.hip.  ctx lock held throughout.
#pragma once

#include "sg_internal.h"

namespace sg {

// Sorted keys -> flags[i] = a run of equal keys starts at i, pos = the flags'
// scan ([n + 1]: pos[n] is the number of distinct keys) and, unless u is null,
// the distinct keys, ascending, in u.  The scan takes the workspace from `tail`.
int rank_runs(sg_ctx* ctx, const uint64_t* sorted, uint64_t n, uint32_t* flags, uint64_t* pos, uint64_t* u,
              size_t tail);

// The general path's workspace: ng values in v with a copy in ka, a second key
// buffer kb, pos [ng + 1], flags [ng], and the workspace past `tail` for the
// sort and the scan.  rank_ws adds these regions to a plan whose other regions
// its caller has added already (tail is the plan's end) and binds them;
// rank_ws_bytes is what they, the sort and the scan take.
struct RankWs {
  uint64_t ng;
  uint64_t *v, *ka, *kb, *pos;
  uint32_t* flags;
  size_t tail;
};
RankWs rank_ws(sg_ctx* ctx, WsPlan& p, uint64_t ng);
size_t rank_ws_bytes(uint64_t ng);

// g.v (and its copy in g.ka) -> the distinct values u, ascending (their number
// at g.pos[ng]), and each value's rank among them.  vary: the bits that differ
// between values (the sort's passes).
int rank_values(sg_ctx* ctx, const RankWs& g, uint64_t vary, uint64_t* u, uint32_t* rank);
// g.v = g.ka = hi << 32 | lo
int rank_pack(sg_ctx* ctx, const RankWs& g, const uint32_t* hi, const uint32_t* lo);

// Groups (calls) over a CSR of `total` members, some flagged for the general
// path, group c's members at places gbase[c] .. of ng.
// rank_flag_all: every group is flagged, in place (gbase = its clamped offset);
// with sel ([ngroups], nullable; cover alone passes one) every selected group
// that has members, at a place taken as the fast shapes' flagged groups take
// theirs: scal = {flagged groups, their members}.
int rank_flag_all(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* sel, uint8_t* flag,
                  uint64_t* gbase, unsigned long long* scal);
// gidx / ggroup: the member and the group of each of the ng places
int rank_fill(sg_ctx* ctx, const uint64_t* off, uint64_t ngroups, uint64_t total, const uint8_t* flag,
              const uint64_t* gbase, uint64_t ng, uint32_t* gidx, uint32_t* ggroup);
// The sort of ggroup << 32 | rank (*sorted), its first occurrences (g.flags)
// with their scan (g.pos), and each group's first place among them (first,
// [ngroups]).
int rank_group_first(sg_ctx* ctx, const RankWs& g, const uint32_t* ggroup, const uint32_t* rank, uint64_t ngroups,
                     uint64_t* first, uint64_t** sorted);

// ws_reserve, then `redo` when the workspace grew: growing drops the contents,
// so what an earlier pass left there went with it.
template <typename Redo>
int ws_reserve_redo(sg_ctx* ctx, size_t bytes, Redo&& redo) {
  const size_t had = ctx->ws.cap;
  const int rc = ws_reserve(ctx, bytes);
  if (rc) return rc;
  return ctx->ws.cap != had ? redo() : SG_OK;
}

// A call with a fast shape and a general path, up to the general path itself.
// first_pass() binds the caller's pointers to the workspace, zeroes its front
// and flags the groups: all of them (all_general) or those its fast shapes
// cannot hold, leaving {flagged groups, their members} at scal_off.  The
// workspace holds `need` bytes for it and general_bytes(ng) more for a general
// path over ng members.  On return *ng is the general path's members (0: there
// is no general path to run), *general the flagged groups, and the workspace
// holds the first pass's results and room for both.
struct TwoPath {
  bool all_general;  // the option: every (selected) group takes the general path
  bool selected;     // ... only the groups of a selection mask, so their members have to be read
  uint64_t ngroups, members;
  uint64_t fast_cap;  // distinct members a group may hold on the fast shape
  size_t need, scal_off;
};
template <typename FirstPass, typename GeneralBytes>
int two_path_first(sg_ctx* ctx, const TwoPath& t, FirstPass&& first_pass, GeneralBytes&& general_bytes, uint64_t* general,
                   uint64_t* ng) {
  *ng = 0;
  int rc = ws_reserve(ctx, t.all_general ? t.need + general_bytes(t.members) : t.need);
  if (rc) return rc;
  if ((rc = first_pass())) return rc;
  if (t.all_general && !t.selected) {
    *ng = t.members;
    *general = t.ngroups;
    return SG_OK;
  }
  // No group of a batch of at most fast_cap members can be flagged by a fast
  // shape: such a batch is read by nobody.
  if (!t.all_general && t.members <= t.fast_cap) return SG_OK;
  // the one device-to-host read (16 B, one wait): the flagged groups' members
  // size the general path's workspace
  unsigned long long got[2] = {0, 0};
  SG_HIP(hipMemcpyAsync(got, ws_at(ctx, t.scal_off), sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *general = got[0];
  *ng = got[1] <= t.members ? got[1] : t.members;
  if (*ng == 0) return SG_OK;
  return ws_reserve_redo(ctx, t.need + general_bytes(*ng), first_pass);
}

}  // namespace sg
