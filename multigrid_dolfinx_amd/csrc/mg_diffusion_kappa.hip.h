// kappa coarsened on the device for gfx950, and in the same pass over the fine field the copy a matrix-free level keeps
// of a kappa it does not own (mg_gen_diffusion_hierarchy[_mf | _device], mg_refresh_diffusion_hierarchy).
//
// kappa_ingest<DIM> reads the fine kappa once -- the top level's upload or the caller's device buffer, the result of the
// level above below it -- and writes
//   * the coarse kappa (N_c = N_f / 2 cells per dimension): the 2^DIM children in ascending lexicographic order, i.e.
//     3-D (z, y, x) = (2ck + c, 2cj + b, 2ci + a) and 2-D (y, x) = (2ck + b, 2ci + a) with a fastest, summed one by one
//     into one accumulator that starts at 0.0, then x 2^-DIM (harmonic == 0) or 2^DIM / sum of 1 / kappa
//     (harmonic == 1).  poisson.coarsen_kappa restates it, and the tests hold the kernel to it bit for bit;
//   * the fine level's own copy (fine_out != nullptr: the level is matrix-free and does not own the source).
// Built with -ffp-contract=off like everything else.
//
// One thread owns one coarse cell and loads its children as x-adjacent pairs: the pair (2 ci, 2 ci + 1) of a fine line
// starts at an even index, so with 16-byte aligned buffers (vec == 1) it is one 16-byte load and, for the copy, one
// 16-byte store, and the threads of a wave read and write contiguous kilobytes per child line.  Buffers that are not
// 16-byte aligned (a view into a caller's tensor) take the same path with two 8-byte accesses per pair (vec == 0).
// Grid-stride loop over the coarse cells, 64-bit indices, no LDS.
// Model: 8 B read + 8 B written (the copy) + 2^-DIM * 8 B written per fine cell: 17 B in 3-D with the copy, 9 B without.
#pragma once
#include "mg_kernels.hip.h"

namespace mgk {

constexpr int KI_BLOCK = 256;

template <int DIM>
__global__ __launch_bounds__(KI_BLOCK) void kappa_ingest(const double* __restrict__ fine, double* __restrict__ fine_out,
                                                         double* __restrict__ coarse, int Nc, int harmonic, int vec) {
    const int64_t nc = DIM == 3 ? (int64_t)Nc * Nc * Nc : (int64_t)Nc * Nc;
    const int64_t Nf = 2 * (int64_t)Nc;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ci = q % Nc;
        const int64_t cj = DIM == 3 ? (q / Nc) % Nc : 0;
        const int64_t ck = DIM == 3 ? q / ((int64_t)Nc * Nc) : q / Nc;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < (DIM == 3 ? 2 : 1); ++c)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                // 3-D: (z, y, x) = (2ck + c, 2cj + b, 2ci); 2-D: (y, x) = (2ck + b, 2ci): the pair a = 0, 1
                const int64_t f = DIM == 3 ? ((2 * ck + c) * Nf + 2 * cj + b) * Nf + 2 * ci : (2 * ck + b) * Nf + 2 * ci;
                double2 x;
                if (vec) {
                    x = *reinterpret_cast<const double2*>(fine + f);
                    if (fine_out) *reinterpret_cast<double2*>(fine_out + f) = x;
                } else {
                    x.x = fine[f];
                    x.y = fine[f + 1];
                    if (fine_out) {
                        fine_out[f] = x.x;
                        fine_out[f + 1] = x.y;
                    }
                }
                s = s + (harmonic ? 1.0 / x.x : x.x);
                s = s + (harmonic ? 1.0 / x.y : x.y);
            }
        coarse[q] = harmonic ? (DIM == 3 ? 8.0 : 4.0) / s : s * (DIM == 3 ? 0.125 : 0.25);
    }
}

}  // namespace mgk
