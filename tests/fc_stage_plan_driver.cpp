// Prints the out-of-place alt rows the segment planner (expecto_amd/csrc/seg_plan.h) gives the Karatsuba
// FC1 slices of segment-pair calls, for tests/test_fc_stage_plan.py.
// stdin: cases of whitespace-separated integers until EOF,
//   n_seg L mode n_win max_batch fk_cap inplace  win_seg[n_win] win_off[n_win] var_pos[n_seg]
// stdout per case: "case", then "error <message>" or "fkm <0/1>", "n_ph <n>" and per chunk and slice
//   "slice <chunk> <i0> <i1> <n_ag> <nw_pre>"
//   "win <w> <block> <conv6 offset> <is alt> <r6 of its block>"   per window of the slice, in order
//   "grp <product> <slab> <group indices>"                        18 lines (slices with alt groups)
//   "alt <slice indices of the alt windows>", "tail <slice indices of the reached tails>"
// then "end".
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
  long long n_seg, L, mode, n_win, max_batch, fk_cap, inplace;
  while (std::cin >> n_seg >> L >> mode >> n_win >> max_batch >> fk_cap >> inplace) {
    std::vector<int> win_seg(n_win), win_off(n_win), var_pos(n_seg);
    for (auto* v : {&win_seg, &win_off, &var_pos})
      for (int& x : *v) std::cin >> x;
    SegPlanIn in{(int)n_seg, (int)L, (int)mode, win_seg.data(), win_off.data(), nullptr, (int)n_win, var_pos.data(),
                 2 * n_win, (int)max_batch, (size_t)max_batch * 1996 * 320, (size_t)max_batch * 496 * 320, true, 0, true,
                 fk_cap};
    in.alt_inplace = inplace != 0;
    SegPlan p;
    const char* err = nullptr;
    std::printf("case\n");
    if (seg_plan(in, p, &err)) {
      std::printf("error %s\nend\n", err);
      continue;
    }
    line("fkm", std::vector<int>{p.fkm});
    line("n_ph", std::vector<int>{p.n_ph});
    for (size_t ci = 0; p.fkm && ci < p.chunks.size(); ++ci) {
      const std::vector<FkWin>& ws = p.fk_ref[ci];
      FkSlice s{};
      for (size_t i0 = 0; i0 < ws.size(); i0 = s.i1) {
        if (const char* refusal = p.fk_slice(ci, i0, s)) {
          std::printf("error %s\n", refusal);
          break;
        }
        line("slice", std::vector<long long>{(long long)ci, (long long)s.i0, (long long)s.i1, s.n_ag, (long long)s.nw_pre});
        for (size_t i = s.i0; i < s.i1; ++i)
          line("win", std::vector<int>{ws[i].w, ws[i].blk, ws[i].off6, p.v_is_alt(ws[i].w),
                                       p.pairs ? p.r6[(size_t)p.chunks[ci].first * p.n_ph + ws[i].blk] : -1});
        if (s.n_ag == 0) continue;
        const FkAltPlan a = p.fk_alt_plan(ci, s);
        for (int g = 0; g < 9; ++g)
          for (int sb = 0; sb < kFkSlabs; ++sb) {
            std::vector<int> l{g, sb};
            l.insert(l.end(), a.grp[g][sb].begin(), a.grp[g][sb].end());
            line("grp", l);
          }
        line("alt", a.win);
        line("tail", a.tail);
      }
    }
    std::printf("end\n");
  }
  return 0;
}
