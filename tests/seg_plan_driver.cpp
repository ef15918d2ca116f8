// Prints the segment path's plans (expecto_amd/csrc/seg_plan.h) as text, for tests/test_seg_plan.py.
// stdin: cases of whitespace-separated integers until EOF,
//   n_seg L mode n_win has_var has_row max_batch p_cap q_cap merge chunk_windows fk fk_cap rc_rows
//   win_seg[n_win] win_off[n_win] (win_row[n_win]) (var_pos[n_seg])
// stdout per case: "case", then "error <message>" or one "<name> <integers>" line per plan field and,
// per chunk, its Karatsuba tables: the windows in group order as (w, block, conv6 offset, group
// start) and the slices as (i0, i1, n_ag, nw_pre); then "end".
#include <cstdio>
#include <iostream>
#include <vector>

#include "../expecto_amd/csrc/seg_plan.h"

using namespace expecto;

template <class V>
static void line(const char* name, const V& v) {
  std::printf("%s", name);
  for (auto x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}

int main() {
  long long n_seg, L, mode, n_win, has_var, has_row, max_batch, p_cap, q_cap, merge, chunk_windows, fk, fk_cap, rc_rows;
  while (std::cin >> n_seg >> L >> mode >> n_win >> has_var >> has_row >> max_batch >> p_cap >> q_cap >> merge >>
         chunk_windows >> fk >> fk_cap >> rc_rows) {
    std::vector<int> win_seg(n_win), win_off(n_win), win_row(has_row ? n_win : 0), var_pos(has_var ? n_seg : 0);
    for (auto* v : {&win_seg, &win_off, &win_row, &var_pos})
      for (int& x : *v) std::cin >> x;
    const SegPlanIn in{(int)n_seg, (int)L, (int)mode, win_seg.data(), win_off.data(), has_row ? win_row.data() : nullptr,
                       (int)n_win, has_var ? var_pos.data() : nullptr, rc_rows, (int)max_batch, (size_t)p_cap,
                       (size_t)q_cap, merge != 0, (int)chunk_windows, fk != 0, fk_cap};
    SegPlan p;
    const char* err = nullptr;
    std::printf("case\n");
    if (seg_plan(in, p, &err)) {
      std::printf("error %s\nend\n", err);
      continue;
    }
    const SegGeo& g = p.g;
    line("present", std::vector<int>(p.present, p.present + 4));
    line("n_ph", std::vector<int>{p.n_ph});
    line("ph", std::vector<int>(p.ph, p.ph + 4));
    line("ph_idx", std::vector<int>(p.ph_idx, p.ph_idx + 4));
    line("geo", std::vector<long long>{g.L, g.T1, g.S1, g.P1, g.T3, g.T4, g.S5, g.T5, g.T6, (long long)g.p_rows_floats,
                                       (long long)g.q_rows_floats});
    line("seg_cap", std::vector<int>{p.seg_cap});
    line("ss", std::vector<long long>{p.ss.n_seg, p.ss.rc_ent, p.ss.n_win, p.ss.rc_win, p.ss.rc_rows});
    line("n_ent", std::vector<int>{p.n_ent});
    line("n_vw", std::vector<int>{p.n_vw});
    line("blk_per_seg", std::vector<int>{p.blk_per_seg});
    line("fkm", std::vector<int>{p.fkm});
    line("first", p.first);
    line("vfirst", p.vfirst);
    line("is_alt", p.is_alt);
    line("alt_w", p.alt_w);
    line("copy_w", p.copy_w);
    std::vector<int> ch;
    for (const auto& c : p.chunks) {
      ch.push_back(c.first);
      ch.push_back(c.second);
    }
    line("chunks", ch);
    line("fc_perm", p.fc_perm);
    for (size_t ci = 0; p.fkm && ci < p.chunks.size(); ++ci) {
      std::vector<int> ref, alt, sl;
      for (const FkWin& w : p.fk_ref[ci])
        for (int x : {w.w, w.blk, w.off6, fk_group_of(w.off6)}) ref.push_back(x);
      for (const FkWin& w : p.fk_alt[ci]) alt.push_back(w.w);
      line("fk_ref", ref);
      line("fk_alt", alt);
      line("gres", p.fk_gres(ci));
      FkSlice s{};
      const char* refusal = nullptr;
      for (size_t i0 = 0; i0 < p.fk_ref[ci].size() && !(refusal = p.fk_slice(ci, i0, s)); i0 = s.i1)
        for (long long x : {(long long)s.i0, (long long)s.i1, (long long)s.n_ag, (long long)s.nw_pre}) sl.push_back((int)x);
      line("slices", sl);
      if (refusal) std::printf("slice_error %s\n", refusal);
    }
    std::printf("end\n");
  }
  return 0;
}
