// mioc_sdt_plan.h -- the staging layout of a pyramid / separable-transform DP as pure arithmetic: no HIP, no context
// (tests/test_sdt_plan.py compiles it with the host compiler alone).
#pragma once

#include <algorithm>
#include <cstddef>

namespace mioc {

struct SdtPlan {
  bool persist = false;  // one persistent launch (k_sdt_run); else one launch per step over two staging buffers
  int nwg = 0;           // persistent: resident row workgroups, nwg / K per subproblem
  bool one_row = false;  // persistent: nwg = K·B, every workgroup owns one row for the whole launch (k_sdt_run1)
  int nbuf = 2;          // staging buffers per subproblem
  size_t s_stride = 0;   // doubles of one staging buffer: (B + 1)·L
  size_t kstride = 0;    // doubles between two subproblems' staging blocks
};

// opt_persist: the caller wants the persistent driver (MIOC_OPT_PERSIST, and the separable transform: the pyramid has
// none); bmax: the largest b̃ of the inputs; ncu x blocks_per_cu: the device's resident row workgroups.
inline SdtPlan sdt_stage_plan(size_t K, size_t nt, int B, size_t L, int M, int bmax, int opt_nb, bool opt_persist,
                              bool force_steps, int ncu, int blocks_per_cu) {
  SdtPlan p;
  p.s_stride = (size_t)(B + 1) * L;
  // persistent separable transform: rows 1..B of every subproblem in contiguous chunks over resident workgroups
  // (one per CU: the row body needs 2 waves per SIMD of registers and ~106 KB of LDS), row 0 of every step
  // precomputed (k_sdt_chain, k_sdt_row0), NB staging buffers
  // (B + 1)·L·8 < 2^31: the persistent kernel addresses a staging block with 32-bit buffer offsets
  // ... and every b̃ within the kernel's dependency window (7 per dimension: u_old on the level grid); a u_old
  // off the grid reaches rows further back than the window waits for, so those problems take per-step launches
  if (opt_persist && nt >= 2 && B >= 1 && p.s_stride * sizeof(double) < (1ull << 31) && bmax <= 7 * M &&
      !force_steps) {
    // one workgroup per CU over contiguous row chunks (k_sdt_run)
    const size_t slots = (size_t)ncu * (size_t)std::max(std::min(blocks_per_cu, 1), 0);
    const size_t per_k = std::min<size_t>((size_t)B, K ? slots / K : 0);  // workgroups per subproblem
    p.nwg = (int)(per_k * K);
    p.persist = per_k >= 1;
  }
  // persistent layout: per subproblem NB staging buffers of (B+1)·L, then row 0 of every step (nt·L), one region
  // addressed by one buffer resource (< 4 GiB); per-step layout: two buffers of K blocks of (B+1)·L
  // at least 7·M + 1 buffers: item (c', i) waits (write-after-read) for the rows up to 7·M above it to have loaded
  // S_{i+NB}, and (one item ahead) for the rows below it to have finished step i; with NB <= 7·M those waits close a
  // cycle -- (c', i) <- (c'-1, i-1) <- ... <- (c'-NB, i-NB), whose WAR wait needs row c' to have loaded S_i, i.e.
  // item (c', i-1) -- and the DP deadlocks until the spin limit (tests/test_gpu_c4.py runs 29, 32 and 37)
  const int nb_min = 7 * M + 1;
  p.nbuf = p.persist ? std::max(opt_nb, nb_min) : 2;
  // one buffer resource addresses a subproblem's whole region (32-bit offsets): as many buffers as fit under 4 GiB
  if (p.persist) {
    const size_t cap = (1ull << 32) / sizeof(double);
    const size_t fit = cap > nt * L ? (cap - nt * L - 1) / p.s_stride : 0;
    if ((size_t)p.nbuf > fit) p.nbuf = (int)fit;
    if (p.nbuf < nb_min) p.persist = false, p.nbuf = 2;  // too few fit to be deadlock-free: per-step launches
  }
  p.kstride = p.persist ? (size_t)p.nbuf * p.s_stride + nt * L : p.s_stride;
  if (p.persist && p.kstride * sizeof(double) >= (1ull << 32)) p.persist = false, p.kstride = p.s_stride;
  p.one_row = p.persist && (size_t)p.nwg == K * (size_t)B;
  return p;
}

}  // namespace mioc
