// The segment path's host planner: which (strand, segment) entries ride in which chunk, the FC row
// order of every chunk and the Karatsuba FC1's slices.  Plain host C++17 on values only -- no HIP, no
// handle -- so a host compiler builds it alone (tests/seg_plan_driver.cpp); forward_segments
// (beluga.hip) fills a SegPlan per call and its stage functions launch by it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

namespace expecto {

constexpr int kLen = 2000;         // input window (chromatin.py:35-36, fixed by FC1)
enum { kStrandFwd = 0, kStrandRc = 1, kStrandBoth = 2 };   // = EXPECTO_STRAND_* (asserted in beluga.hip)

// Strands of a segment call.  Its chunks run over (strand, segment) entries e, the fwd entries first:
// entry e is segment e - n_seg if e >= n_seg, else e, on the rc strand iff e >= rc_ent.  Its windows
// are numbered the same way: v is window v - n_win if v >= n_win (its rows then rc_rows further
// on in the output), else v, on the rc strand iff v >= rc_win.  (FWD: rc_* past every index; RC: 0;
// BOTH: n_seg / n_win.)  A POD, passed to kernels by value.
struct SegStrands {
  int n_seg, rc_ent, n_win, rc_win;
  long long rc_rows;
};

// A segment of L codes (L % 4 == 0); a window at offset o (o % 4 == 0, o + 2000 <= L).
// conv1..conv4 run once over the segment; pool1 is fused into conv2 (phase 0 serves every
// window since o % 4 == 0); pool2 runs separately for each phase p = (o/4) % 4 present;
// conv5/conv6 run per (segment, phase) block; FC1 reads each window's 106 conv6 rows
// through a row table.  Every per-window output element is computed with the same operands
// and K order as the per-window path, so results are bit-identical to it.
struct SegGeo {
  int L, T1, S1, P1, T3, T4, S5, T5, T6;
  size_t p_rows_floats, q_rows_floats;  // per segment, given n_ph phases
};

inline SegGeo seg_geo(int L, int n_ph) {
  SegGeo g{};
  g.L = L;
  g.T1 = L - 7;
  g.S1 = (g.T1 + 3) / 4 * 4;
  g.P1 = (g.T1 - 7) / 4;
  g.T3 = g.P1 - 7;
  g.T4 = g.T3 - 7;
  g.S5 = g.T4 / 4;        // rows of the phase-0 pool2 block (the longest)
  g.T5 = g.S5 - 7;
  g.T6 = g.T5 - 7;
  const size_t p_conv1 = (size_t)g.S1 * 320, p_conv3 = (size_t)((g.T3 + 3) & ~3) * 480, p_pool2 = (size_t)n_ph * g.S5 * 480,
               p_conv6 = (size_t)n_ph * g.T6 * 640;
  const size_t q_pool1 = (size_t)g.P1 * 320, q_conv4 = (size_t)g.T4 * 480, q_conv5 = (size_t)n_ph * g.T5 * 640;
  g.p_rows_floats = std::max(std::max(p_conv1, p_conv3), std::max(p_pool2, p_conv6));
  g.q_rows_floats = std::max(q_pool1, std::max(q_conv4, q_conv5));
  return g;
}

// A window of the segment path for the Karatsuba FC1 (w: its number; off: its offset in its segment,
// chunk block `seg`, strand rc): its conv6 block (seg, pool2 phase) and
// offset in conv6 rows (as seg_a_rows computes them); its role is its 25-row step mod 4 and its
// group the windows of its block with the same group start off6 - 25 role.
struct FkWin {
  int w, blk, off6;
};
inline int fk_role_of(int off6) { return (off6 / 25) & 3; }
inline int fk_group_of(int off6) { return off6 - 25 * fk_role_of(off6); }
inline FkWin fk_win(int w, int seg, int off, bool rc, int L, int n_ph, const int* ph_idx) {
  const int o = rc ? L - kLen - off : off;
  const int q = o >> 2, p = q & 3;
  return {w, seg * n_ph + ph_idx[p], (q - p) >> 2};
}
inline bool fk_same_group(const FkWin& a, const FkWin& b) {
  return a.blk == b.blk && fk_group_of(a.off6) == fk_group_of(b.off6);
}

// The block-Karatsuba FC1's products (beluga.hip, "FC1 as a block-Karatsuba convolution"): product g
// reads one sequence at one 25-row block of its group, in kFkSlabs K slabs; a window in role a sums
// the products kFkRole[a].
constexpr int kFkK = 16000;                              // one 25-row block of conv6 rows (25 x 640)
constexpr int kFkSlabs = 2;                              // K slabs per product
constexpr int kFkSeq[9] = {3, 2, 3, 1, 0, 1, 3, 2, 3};   // product g reads sequence (0 x, 1 D1, 2 D2, 3 DD)
constexpr int kFkBlk[9] = {0, 1, 1, 2, 3, 3, 2, 3, 3};   //   at block kFkBlk[g] of its group
constexpr int kFkRole[4][4] = {{0, 1, 3, 4}, {1, 2, 4, 5}, {3, 4, 6, 7}, {4, 5, 7, 8}};

// Segment pairs: the first changed conv6 row of a (segment, pool2 phase p) block whose SNV is at
// base q of the segment in the block's strand orientation -- seg_delta_table's arithmetic (beluga.hip)
// on the host.  The alt block differs from the ref block in rows [r6, r6 + kSegW6) only.
constexpr int kSegW[7] = {0, 8, 5, 12, 19, 6, 13};       // run widths: conv1, conv2+pool1, conv3, conv4, pool2, conv5
constexpr int kSegW6 = 20;                               //   and conv6
inline int seg_floor4(int v) { return v >= 0 ? v >> 2 : -((3 - v) >> 2); }
inline int seg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline int seg_r6(const SegGeo& g, int q, int p) {
  const int r1 = seg_clamp(q - 7, 0, g.T1 - kSegW[1]);
  const int r2 = seg_clamp(seg_floor4(r1 - 7), 0, g.P1 - kSegW[2]);
  const int r3 = seg_clamp(r2 - 7, 0, g.T3 - kSegW[3]);
  const int r4 = seg_clamp(r3 - 7, 0, g.T4 - kSegW[4]);
  const int r4p = seg_clamp(seg_floor4(r4 - p), 0, g.S5 - kSegW[5]);
  const int r5 = seg_clamp(r4p - 7, 0, g.T5 - kSegW[6]);
  return seg_clamp(r5 - 7, 0, g.T6 - kSegW6);
}

// Does the partial (product g, K slab s) of the group that starts at conv6 row G read a changed row
// of its block, [r6, r6 + kSegW6)?  The slab's rows of the product's block, with the lags of its
// sequence (D1: 25; D2: 50; DD: 25, 50, 75).  The tail of a window at off6 reads rows 100..105.
inline bool fk_reach(int G, int g, int s, int r6) {
  const int base = G + 25 * kFkBlk[g], per = kFkK / kFkSlabs;
  const int i0 = base + (s * per) / 640, i1 = base + ((s + 1) * per - 1) / 640;
  const int sq = kFkSeq[g], nl = sq == 0 ? 1 : sq == 3 ? 4 : 2, lag1 = sq == 2 ? 50 : 25;
  bool hit = false;
  for (int l = 0; l < nl; ++l) {
    const int lag = l == 0 ? 0 : (nl == 2 ? lag1 : 25 * l);
    hit |= i0 + lag < r6 + kSegW6 && i1 + lag >= r6;
  }
  return hit;
}
inline bool fk_reach_tail(int off6, int r6) { return off6 + 100 < r6 + kSegW6 && off6 + 105 >= r6; }

// What a segment call is planned from: the caller's host tables and the handle's sizes and knobs.
struct SegPlanIn {
  int n_seg, L, mode;                          // mode: kStrandFwd / Rc / Both
  const int *win_seg, *win_off, *win_row;      // win_row may be null
  int n_win;
  const int* var_pos;                          // segment pairs: the SNV's position per segment; else null
  long long rc_rows;                           // output rows between the strands (SegStrands)
  int max_batch;
  size_t p_cap, q_cap;                         // elements of the P / Q workspaces that hold segment rows
  bool merge_strands;                          // EXPECTO_SEG_MERGE_STRANDS
  int chunk_windows;                           // EXPECTO_SEG_CHUNK_WINDOWS (<= 0: no cap)
  bool fk;                                     // the Karatsuba FC1 is on for segments
  long long fk_cap;                            // windows per Karatsuba FC1 slice
  bool alt_inplace = false;                    // EXPECTO_FC1K_ALT_INPLACE: the alt FC1 as a pass of its own
};

// A slice [i0, i1) of a chunk's group order and its leading groups that hold an alt window: n_ag
// groups, the slice's first nw_pre windows.
struct FkSlice {
  size_t i0, i1, nw_pre;
  int n_ag;
};

// The alt work of a slice as rows of its grouped FC1 launch (segment pairs, out of place): per
// product g and K slab s the alt groups (k-th group of the slice, k < n_ag) whose partial an alt
// window sums and a changed conv6 row reaches; the alt windows (index in the slice, < nw_pre) and
// those whose tail is reached.  Every other partial of an alt window is its ref partial, bit for bit.
struct FkAltPlan {
  std::vector<int> grp[9][kFkSlabs];
  std::vector<int> win, tail;
};

struct SegPlan {
  int present[4], n_ph, ph[4], ph_idx[4];      // pool2 phases in the computed strands' coordinates
  SegGeo g;
  int seg_cap;                                 // entries whose rows the workspaces hold
  SegStrands ss;
  int n_ent, n_vw;                             // (strand, segment) entries and their windows
  int blk_per_seg;                             // alt-run blocks per entry (0: no pairs)
  bool pairs;
  std::vector<int> first, vfirst;              // first window of segment s / of entry e
  std::vector<char> is_alt;                    // window w holds its segment's SNV
  std::vector<int> alt_w, copy_w;              // window numbers v, ascending
  std::vector<std::pair<int, int>> chunks;     // entries [first, second)
  std::vector<int> fc_perm;                    // FC row order: pair order [n_vw], or group order (fkm) [4 n_win]
  bool fkm;                                    // FC1 as the block Karatsuba
  std::vector<std::vector<FkWin>> fk_ref, fk_alt;   // [chunk]: its windows in group order; its alt windows
  long long fk_cap;
  bool alt_inplace;
  std::vector<int> r6;                         // pairs: first changed conv6 row of block (entry e, phase index i) at e * n_ph + i

  int vw_w(int v) const { return v >= ss.n_win ? v - ss.n_win : v; }
  bool v_is_alt(int v) const { return is_alt[vw_w(v)] != 0; }

  // per conv6 block of chunk ci: its groups' start residue mod 100 (all equal on 200-bp sweeps), so the
  // sequences are formed only on the rows the products read; -1: they differ; -2: a block no window reads
  std::vector<int> fk_gres(size_t ci) const {
    std::vector<int> gres((size_t)(chunks[ci].second - chunks[ci].first) * n_ph, -2);
    for (const FkWin& w : fk_ref[ci]) {
      const int r = fk_group_of(w.off6) % 100;
      int& e = gres[(size_t)w.blk];
      e = e == -2 ? r : (e == r ? r : -1);
    }
    return gres;
  }

  // The slice of chunk ci's group order that starts at i0: whole groups, <= fk_cap windows, and its
  // alt-group prefix (the alt groups lead the chunk's order, so they fill the first slices).
  // Out of place, an alt window counts twice (its ref and its alt FC1 output row share the slice's
  // buffers); the first group of a slice is taken whatever it counts.  Returns the refusal, or null.
  const char* fk_slice(size_t ci, size_t i0, FkSlice& s) const {
    const std::vector<FkWin>& ws = fk_ref[ci];
    const bool twice = pairs && !alt_inplace && !fk_alt[ci].empty();
    size_t i1 = i0, rows = 0;
    while (i1 < ws.size()) {
      size_t j = i1, n = 0;
      do n += twice && v_is_alt(ws[j].w) ? 2 : 1;
      while (++j < ws.size() && fk_same_group(ws[j], ws[i1]));
      if (rows + n > (size_t)fk_cap && i1 > i0) break;
      rows += n;
      i1 = j;
    }
    if (i1 - i0 > (size_t)fk_cap) return "a Karatsuba FC1 window group exceeds the FC1 slice";
    s = {i0, i1, 0, 0};
    const bool has_alt = pairs && !fk_alt[ci].empty();
    for (size_t i = i0; has_alt && i < i1; ++i) {
      bool galt = false;
      size_t j = i;
      for (; j < i1 && fk_same_group(ws[j], ws[i]); ++j) galt |= v_is_alt(ws[j].w);
      if (!galt) break;
      ++s.n_ag;
      s.nw_pre = j - i0;
      i = j - 1;
    }
    return nullptr;
  }

  // The out-of-place alt rows of slice s of chunk ci (s.n_ag > 0)
  FkAltPlan fk_alt_plan(size_t ci, const FkSlice& s) const {
    const std::vector<FkWin>& ws = fk_ref[ci];
    FkAltPlan a;
    int k = -1;
    for (size_t i = s.i0; i < s.i0 + s.nw_pre; ++i) {
      if (i == s.i0 || !fk_same_group(ws[i], ws[i - 1])) ++k;
      const FkWin& w = ws[i];
      if (!v_is_alt(w.w)) continue;
      const int r = r6[(size_t)chunks[ci].first * n_ph + w.blk];
      a.win.push_back((int)(i - s.i0));
      if (fk_reach_tail(w.off6, r)) a.tail.push_back((int)(i - s.i0));
      for (int j = 0; j < 4; ++j) {
        const int g = kFkRole[fk_role_of(w.off6)][j];
        for (int sb = 0; sb < kFkSlabs; ++sb) {
          std::vector<int>& l = a.grp[g][sb];   // (k ascends: a group's alt windows are consecutive)
          if (fk_reach(fk_group_of(w.off6), g, sb, r) && (l.empty() || l.back() != k)) l.push_back(k);
        }
      }
    }
    return a;
  }
};

// Plans a segment call.  Returns 0, or -1 with *err the refusal (the caller's tables are wrong, or a
// segment does not fit the workspaces).
inline int seg_plan(const SegPlanIn& in, SegPlan& p, const char** err) {
#define SEG_PLAN_REQUIRE(cond, msg) \
  do {                              \
    if (!(cond)) {                  \
      *err = msg;                   \
      return -1;                    \
    }                               \
  } while (0)
  const int n_seg = in.n_seg, L = in.L, mode = in.mode, n_win = in.n_win;
  const int *win_seg = in.win_seg, *win_off = in.win_off;
  SEG_PLAN_REQUIRE(L >= kLen && L % 4 == 0, "segment length must be >= 2000 and a multiple of 4");
  // phases present (fwd and, for BOTH, the mirrored rc offsets)
  for (int i = 0; i < 4; ++i) p.present[i] = p.ph[i] = p.ph_idx[i] = 0;
  for (int w = 0; w < n_win; ++w) {
    SEG_PLAN_REQUIRE(win_seg[w] >= 0 && win_seg[w] < n_seg, "window segment out of range");
    SEG_PLAN_REQUIRE(w == 0 || win_seg[w] >= win_seg[w - 1], "windows must be sorted by segment");
    const int o = win_off[w];
    SEG_PLAN_REQUIRE(o >= 0 && o % 4 == 0 && o + kLen <= L, "window offset must be 4-aligned inside the segment");
    // phases in the computed strands' coordinates (seg_a_rows: rc windows start at L - 2000 - o)
    if (mode != kStrandRc) p.present[(o >> 2) & 3] = 1;
    if (mode != kStrandFwd) p.present[((L - kLen - o) >> 2) & 3] = 1;
  }
  p.n_ph = 0;
  for (int q = 0; q < 4; ++q)
    if (p.present[q]) {
      p.ph_idx[q] = p.n_ph;
      p.ph[p.n_ph++] = q;
    }
  const int n_ph = p.n_ph;
  p.g = seg_geo(L, std::max(n_ph, 1));
  p.seg_cap = (int)std::min<size_t>(in.p_cap / p.g.p_rows_floats, in.q_cap / p.g.q_rows_floats);
  SEG_PLAN_REQUIRE(p.seg_cap >= 1, "segment too long for this handle's workspace (raise max_batch)");
  // window ranges per segment
  p.first.assign(n_seg + 1, n_win);
  for (int w = n_win - 1; w >= 0; --w) p.first[win_seg[w]] = w;
  for (int sg = n_seg - 1; sg >= 0; --sg) p.first[sg] = std::min(p.first[sg], p.first[sg + 1]);
  // (strand, segment) entries and their windows, the fwd strand's first (SegStrands)
  const int strands = mode == kStrandBoth ? 2 : 1;
  const int n_ent = p.n_ent = strands * n_seg, n_vw = p.n_vw = strands * n_win;
  p.ss = SegStrands{n_seg, mode == kStrandFwd ? n_ent : mode == kStrandRc ? 0 : n_seg,
                    n_win, mode == kStrandFwd ? n_vw : mode == kStrandRc ? 0 : n_win, in.rc_rows};
  p.vfirst.assign(n_ent + 1, n_vw);   // first window of entry e
  for (int e = 0; e < n_ent; ++e) p.vfirst[e] = e >= n_seg ? n_win + p.first[e - n_seg] : p.first[e];
  p.pairs = in.var_pos != nullptr;
  p.is_alt.assign(n_win, 0);
  p.alt_w.clear();
  p.copy_w.clear();
  if (p.pairs) {
    for (int sg = 0; sg < n_seg; ++sg)
      SEG_PLAN_REQUIRE(in.var_pos[sg] >= 0 && in.var_pos[sg] < L, "variant position outside its segment");
    for (int w = 0; w < n_win; ++w) {
      const int q = in.var_pos[win_seg[w]];
      p.is_alt[w] = win_off[w] <= q && q < win_off[w] + kLen;
    }
    for (int v = 0; v < n_vw; ++v) (p.v_is_alt(v) ? p.alt_w : p.copy_w).push_back(v);
  }
  if (in.win_row)
    for (int w = 0; w < n_win; ++w)
      SEG_PLAN_REQUIRE(in.win_row[w] >= 0 && in.win_row[w] < n_win, "window row out of range");
#undef SEG_PLAN_REQUIRE
  // alt runs: one block per segment (conv1..4) or per (segment, phase) (pool2, conv5, conv6)
  p.blk_per_seg = p.pairs ? std::max(n_ph, 1) : 0;
  // chunks of whole (strand, segment) entries: grow while the segment buffers and the alt-run
  // buffers (<= max_batch blocks) fit.  The FC stage of a chunk runs in slices of <= max_batch
  // windows (its workspace), so a chunk is not bounded by its window count: one large chunk instead
  // of several keeps every conv launch's last partial round of 256 workgroups to one per chunk (the
  // 200-window workload: 96 segments per strand in one chunk instead of 40 + 40 + 16), and a chunk
  // runs on across the strand boundary (both strands' 192 entries in one chunk: every stage is
  // launched once per step, not once per strand; EXPECTO_SEG_MERGE_STRANDS=0 ends a chunk there)
  p.chunks.clear();
  for (int e0 = 0; e0 < n_ent;) {
    int e1 = e0 + 1;
    while (e1 < n_ent && (e1 != n_seg || in.merge_strands) && e1 - e0 < p.seg_cap &&
           (long long)(e1 + 1 - e0) * p.blk_per_seg <= in.max_batch &&
           (in.chunk_windows <= 0 || p.vfirst[e1 + 1] - p.vfirst[e0] <= in.chunk_windows))
      ++e1;
    p.chunks.push_back({e0, e1});
    e0 = e1;
  }
  // Segment pairs where more than a third of the windows hold the SNV (short sweeps: +-800, every
  // window) run the direct FC1 (role 4): an alt window's Karatsuba products mix rows 25-75 apart, so
  // nearly all of them reach the changed rows and the alt recompute outweighs the saving
  // (configs[2]: 14.4 k vs 16.6 k variants/s); the 200-window sweeps (5 % alt windows) gain.
  p.fkm = in.fk && !(p.pairs && 3 * p.alt_w.size() > (size_t)n_vw);
  p.fk_cap = in.fk_cap;
  p.alt_inplace = in.alt_inplace;
  p.r6.clear();
  if (p.pairs)
    for (int e = 0; e < n_ent; ++e) {
      const int q = in.var_pos[e >= n_seg ? e - n_seg : e];
      for (int i = 0; i < n_ph; ++i) p.r6.push_back(seg_r6(p.g, e >= p.ss.rc_ent ? L - 1 - q : q, p.ph[i]));
    }
  p.fc_perm.clear();
  p.fk_ref.clear();
  p.fk_alt.clear();
  if (p.pairs && !p.fkm) {
    // Segment pairs: the FC rows of a chunk are its alt windows sorted by the SNV's position in
    // the window (in the window's strand orientation), then the other windows.  The ref FC1 runs in
    // that order, and the alt FC1 over the first rows recomputes only the split-K slabs its changed
    // conv6 rows touch (a 256-row tile then holds windows with nearly the same changed rows), reusing
    // the ref partials.
    p.fc_perm.resize((size_t)n_vw);
    auto pos_of = [&](int v) {
      const int w = p.vw_w(v), q = in.var_pos[win_seg[w]] - win_off[w];
      return v >= p.ss.rc_win ? kLen - 1 - q : q;
    };
    for (const auto& c : p.chunks) {
      const int w0 = p.vfirst[c.first], w1 = p.vfirst[c.second];
      int k = w0;
      std::vector<int> a;
      for (int v = w0; v < w1; ++v)
        if (p.v_is_alt(v)) a.push_back(v);
      std::stable_sort(a.begin(), a.end(), [&](int x, int y) { return pos_of(x) < pos_of(y); });
      for (int v : a) p.fc_perm[k++] = v;
      for (int v = w0; v < w1; ++v)
        if (!p.v_is_alt(v)) p.fc_perm[k++] = v;
    }
  }
  if (p.fkm) {
    // FC1 as the block Karatsuba (f16x3): per chunk the windows in group order (conv6 block, group
    // start, role), the FC order of every launch and (segment pairs) the alt windows in the same
    // order; fc_perm holds [strand][n_win] FC orders, then [strand][n_win] alt orders
    p.fc_perm.assign((size_t)4 * n_win, 0);
    for (const auto& c : p.chunks) {
      const int w0 = p.vfirst[c.first], w1 = p.vfirst[c.second];
      // group order: (segment pairs) the groups holding an alt window first, ordered by where the
      // SNV falls in the group (so an M tile of the in-place alt FC1 holds groups whose changed
      // products are the same and its masks stay sparse), then every other group; in a group its
      // windows by role
      struct Key {
        int cls;
        long long rel;
        int blk, G, off6, w;
      };
      std::vector<FkWin> ref, alt;
      std::vector<Key> key;
      std::map<std::pair<int, int>, int> galt;   // (block, group start) -> holds an alt window
      for (int v = w0; v < w1; ++v) {   // a group lies in one block, so it never mixes strands
        const int w = p.vw_w(v);
        const FkWin fw = fk_win(v, win_seg[w] + (v >= n_win ? n_seg : 0) - c.first, win_off[w], v >= p.ss.rc_win, L,
                                n_ph, p.ph_idx);
        ref.push_back(fw);
        if (p.pairs && p.v_is_alt(v)) {
          alt.push_back(fw);
          galt[{fw.blk, fk_group_of(fw.off6)}] = 1;
        }
      }
      for (const FkWin& fw : ref) {
        const int G = fk_group_of(fw.off6);
        const bool ga = p.pairs && galt.count({fw.blk, G});
        long long rel = 0;
        if (ga) {
          const int q = in.var_pos[win_seg[p.vw_w(fw.w)]];
          rel = (long long)(fw.w >= p.ss.rc_win ? L - 1 - q : q) - 16LL * G;
        }
        key.push_back({ga ? 0 : 1, rel, fw.blk, G, fw.off6, fw.w});
      }
      std::vector<int> ord(ref.size());
      for (size_t k = 0; k < ord.size(); ++k) ord[k] = (int)k;
      std::sort(ord.begin(), ord.end(), [&](int a, int b) {
        const Key &x = key[a], &y = key[b];
        return std::tie(x.cls, x.rel, x.blk, x.G, x.off6, x.w) < std::tie(y.cls, y.rel, y.blk, y.G, y.off6, y.w);
      });
      std::vector<FkWin> sorted;
      for (int k : ord) sorted.push_back(ref[k]);
      for (size_t k = 0; k < sorted.size(); ++k) p.fc_perm[(size_t)w0 + k] = sorted[k].w;
      p.fk_ref.push_back(std::move(sorted));
      p.fk_alt.push_back(std::move(alt));
    }
  }
  return 0;
}

}  // namespace expecto
