// Host check of ffmi::mid_xcd_map (ffmi_internal.h): the block renumbering of
// split-K M-split GEMM launches.  Built and run by tests/test_mid_xcd_map.py.
// Over nblk 1..130, S 1..8, mblocks 1..3 (grid (nblk, S, mblocks), XCD residue
// = linear block id % 8, x fastest):
//  1. the map is a bijection onto the grid (z untouched), the identity at S = 1;
//  2. S in {2, 4, 8} and nblk % 8 == 0: every residue sees exactly
//     max(1, S / 8) slices and every slice exactly max(1, 8 / S) residues;
//  3. blocks that differ only in z have equal residues wherever they have
//     them under the identity numbering.
#include <cstdio>
#include <vector>

#include "../flexflow_amd/csrc/ffmi_internal.h"

static int fails = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (fails++ < 20) {                   \
        std::printf("FAIL %s: ", #cond);    \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
    }                                       \
  } while (0)

int main() {
  long grids = 0;
  for (int nblk = 1; nblk <= 130; ++nblk)
    for (int S = 1; S <= 8; ++S)
      for (int mb = 1; mb <= 3; ++mb) {
        ++grids;
        const int P = nblk * S;
        // residue of the workgroup that computes logical block (cb, ks, z)
        std::vector<int> res(P * mb, -1);
        for (int z = 0; z < mb; ++z)
          for (int by = 0; by < S; ++by)
            for (int bx = 0; bx < nblk; ++bx) {
              int cb = -1, ks = -1;
              ffmi::mid_xcd_map(bx, by, nblk, S, cb, ks);
              CHECK(cb >= 0 && cb < nblk && ks >= 0 && ks < S, "range nblk %d S %d: (%d, %d) -> (%d, %d)",
                    nblk, S, bx, by, cb, ks);
              if (cb < 0 || cb >= nblk || ks < 0 || ks >= S) continue;
              if (S == 1) CHECK(cb == bx && ks == by, "identity nblk %d", nblk);
              int &slot = res[cb + nblk * (ks + S * z)];
              CHECK(slot == -1, "bijection nblk %d S %d mb %d: (%d, %d) taken twice", nblk, S, mb, cb, ks);
              slot = (bx + nblk * (by + S * z)) & 7;
            }
        for (int i = 0; i < P * mb; ++i) CHECK(res[i] >= 0, "onto nblk %d S %d mb %d: %d unassigned", nblk, S, mb, i);
        if ((S == 2 || S == 4 || S == 8) && nblk % 8 == 0) {
          const int want_s = S / 8 > 1 ? S / 8 : 1, want_r = 8 / S > 1 ? 8 / S : 1;
          int slices_of[8] = {0}, residues_of[8] = {0};  // bit sets
          for (int z = 0; z < mb; ++z)
            for (int ks = 0; ks < S; ++ks)
              for (int cb = 0; cb < nblk; ++cb) {
                const int r = res[cb + nblk * (ks + S * z)];
                if (r < 0) continue;
                slices_of[r] |= 1 << ks, residues_of[ks] |= 1 << r;
              }
          for (int r = 0; r < 8; ++r)
            CHECK(__builtin_popcount(slices_of[r]) == want_s, "nblk %d S %d mb %d: residue %d sees %d slices",
                  nblk, S, mb, r, __builtin_popcount(slices_of[r]));
          for (int ks = 0; ks < S; ++ks)
            CHECK(__builtin_popcount(residues_of[ks]) == want_r, "nblk %d S %d mb %d: slice %d on %d residues",
                  nblk, S, mb, ks, __builtin_popcount(residues_of[ks]));
        }
        for (int z1 = 0; z1 < mb; ++z1)
          for (int z2 = z1 + 1; z2 < mb; ++z2) {
            // identity numbering: residues differ by (z2 - z1) * P for every block
            if (((z2 - z1) * P) & 7) continue;
            for (int i = 0; i < P; ++i)
              CHECK(res[i + P * z1] == res[i + P * z2], "nblk %d S %d: z %d / %d split block %d", nblk, S, z1,
                    z2, i);
          }
      }
  std::printf("%ld grids, %d failures\n", grids, fails);
  return fails ? 1 : 0;
}
