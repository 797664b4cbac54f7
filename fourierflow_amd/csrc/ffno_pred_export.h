// The prediction export of the Markov routine's test (the torus_kochkov/ffno/predictions configs set `pred_path`): the velocity
// image of a prediction -> vorticity, vx, vy on the pred_size x pred_size grid, one launch per rollout step, and the isotropic
// kinetic-energy spectrum of the exported velocities, one launch per test batch.  Reference routines/grid_2d_markov.py:427-476
// (jax-cfd on the CPU, a Python loop over batch and time) with utils/array.py:50-80 downsample_vorticity_hat, and the spectrum that
// commands/plot.py:256-306 takes of the written file.
//
// ffno_prediction_export_step.  The outputs are TIME-MAJOR, [n_steps][B][m][m]: the launch of step t writes slab t of each and
// nothing else, contiguous stores; the host transposes to the reference's (sample, x, y, time) only when it writes the file.
// With f = X / m = Y / m:
//   f == 1  the reference's else branch (:448-452): the three channels of `vel` are copied, bit for bit.
//   f > 1   the staggered-velocity formulas at the top of ffno_coarsen.h (that header defines entry points of its own, so the rule
//           is restated here as in ffno_kf2d.h), dx = len_x / m, dy = len_y / m:
//               u_c[i][j] = (sum_{b<f} u[f i + f-1][f j + b]) / f      every f-th line along x, the LAST of its block, mean across it
//               v_c[i][j] = (sum_{a<f} v[f i + a][f j + f-1]) / f      the same for v along y
//               w_c[i][j] = (v_c[(i+1) % m][j] - v_c[i][j]) / dx - (u_c[i][(j+1) % m] - u_c[i][j]) / dy
//           vx = u_c, vy = v_c, vort = w_c.  Workgroup (slice, sample) owns R consecutive coarse rows with that header's slicing rule
//           (about 1024 cells): u_c of its R rows and v_c of its R + 1 rows (the halo row below, wrapped) go to LDS, every mean a
//           sequential sum in index order; then one thread per coarse cell differences and stores the three values.
//
// ffno_energy_spectrum.  One workgroup per image on the rfft2 half spectra [m][m/2+1][2] of vx and vy; the definition is in
// include/ffno.h.  Wave w of the four takes the shells s = w, w + 4, ...  A shell meets row r in ONE run of columns [lo, hi)
// (k_x fixed, k_x^2 + c^2 grows with c), whose ends come from a float square root corrected by integer comparisons, so the
// membership of a bin is decided in integers.  Summation order of a shell, fixed: lane l adds the bins of rows l, l + 64, l + 128,
// l + 192 in that order, the columns of a run ascending, one sequential fp32 sum; the 64 lane sums go through the xor butterfly
// (32, 16, ... 1); the result times 1 / (2 m^4) is stored by lane 0.  No atomics, no LDS, every output written once.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace pred_export {

static constexpr int kMaxM = 4096;      // (2 R + 1) m floats of LDS with R = 1: 48 KB
static constexpr int kSpecMinM = 8, kSpecMaxM = 256;

// the slicing rule of ffno_coarsen.h: about 1024 coarse cells per workgroup, at least one row; rows() rows per slice, slices() of them
static inline int rows(int m) {
    const long want = ((long)m * m + 1023) / 1024;
    const int S = want < m ? (int)want : m;
    return (m + S - 1) / S;
}
static inline int slices(int m) { return (m + rows(m) - 1) / rows(m); }

__global__ __launch_bounds__(256) void export_copy_kernel(const float* __restrict__ vel, float* __restrict__ vort,
                                                          float* __restrict__ vx, float* __restrict__ vy, size_t cells) {
    for (size_t c = (size_t)blockIdx.x * 256u + threadIdx.x; c < cells; c += (size_t)gridDim.x * 256u) {
        const float* p = vel + 3 * c;
        vort[c] = p[0];
        vx[c] = p[1];
        vy[c] = p[2];
    }
}

__global__ __launch_bounds__(256) void export_coarsen_kernel(const float* __restrict__ vel, float* __restrict__ vort,
                                                             float* __restrict__ vx, float* __restrict__ vy, int X, int Y, int m,
                                                             int f, int R, float dx, float dy) {
    FFNO_DYN_SMEM(smem);
    float* uc = reinterpret_cast<float*>(smem);      // [R][m]
    float* vc = uc + (size_t)R * m;                  // [R + 1][m]
    const int bidx = blockIdx.y;
    const int i0 = blockIdx.x * R, nr = min(R, m - i0);      // this slice's coarse rows [i0, i0 + nr)
    const float* img = vel + (size_t)bidx * X * Y * 3;
    const float ff = (float)f;
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const float* row = img + ((size_t)(f * (i0 + r) + f - 1) * Y + (size_t)f * j) * 3 + 1;
        float a = 0.f;
        for (int b = 0; b < f; ++b) a += row[3 * b];
        uc[c] = a / ff;
    }
    for (int c = threadIdx.x; c < (nr + 1) * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int i = (i0 + r) % m;                          // r = nr on the last slice: coarse row 0
        const float* col = img + ((size_t)f * i * Y + (size_t)f * j + f - 1) * 3 + 2;
        float a = 0.f;
        for (int k = 0; k < f; ++k) a += col[(size_t)3 * Y * k];
        vc[c] = a / ff;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int jn = j + 1 < m ? j + 1 : 0;
        const size_t e = ((size_t)bidx * m + (i0 + r)) * m + j;
        vort[e] = (vc[c + m] - vc[c]) / dx - (uc[r * m + jn] - uc[c]) / dy;
        vx[e] = uc[c];
        vy[e] = vc[c];
    }
}

// the smallest column c in [0, Nh] with 4 (kx2 + c^2) >= T: the square root proposes, the integer comparisons decide
__device__ __forceinline__ int first_column(int T, int kx2, int Nh) {
    const int D = T - 4 * kx2;
    if (D <= 0) return 0;
    int c = (int)sqrtf(0.25f * (float)D);
    while (4 * c * c < D) ++c;
    while (c > 0 && 4 * (c - 1) * (c - 1) >= D) --c;
    return c < Nh ? c : Nh;
}

__global__ __launch_bounds__(256) void energy_spectrum_kernel(const float2* __restrict__ u_h, const float2* __restrict__ v_h,
                                                              float* __restrict__ E, int m, float scale) {
    const int Nh = m / 2 + 1;
    const float2* u = u_h + (size_t)blockIdx.x * m * Nh;
    const float2* v = v_h + (size_t)blockIdx.x * m * Nh;
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x >> 6; s < Nh; s += 4) {      // wave-uniform: every lane of the wave reaches the butterfly
        const int lo_t = s ? (2 * s - 1) * (2 * s - 1) : 0, hi_t = (2 * s + 1) * (2 * s + 1);
        float a = 0.f;
        for (int r = lane; r < m; r += 64) {
            const int kx = r < m / 2 ? r : r - m;
            const int lo = first_column(lo_t, kx * kx, Nh), hi = first_column(hi_t, kx * kx, Nh);
            for (int c = lo; c < hi; ++c) {
                const float2 p = u[(size_t)r * Nh + c], q = v[(size_t)r * Nh + c];
                const float e = (p.x * p.x + p.y * p.y) + (q.x * q.x + q.y * q.y);
                a += (c == 0 || c == m / 2) ? e : 2.f * e;
            }
        }
        a = wave_sum(a);
        if (lane == 0) E[(size_t)blockIdx.x * Nh + s] = a * scale;
    }
}

static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

}  // namespace pred_export
}  // namespace ffno

extern "C" int ffno_prediction_export_step(const float* vel, float* vort, float* vx, float* vy, int B, int X, int Y, int m,
                                           int n_steps, int t, float len_x, float len_y, void* stream) {
    using namespace ffno::pred_export;
    if (!vel || !vort || !vx || !vy || B <= 0 || X <= 0 || Y <= 0 || m <= 0 || n_steps <= 0 || t < 0 || t >= n_steps ||
        !(len_x > 0.f) || !(len_y > 0.f))
        return FFNO_EINVAL;
    if (X % m || Y % m || X / m != Y / m || m > kMaxM || B > 65535) return FFNO_EUNSUPPORTED;
    const size_t slab = (size_t)B * m * m, off = (size_t)t * slab;
    const int f = X / m;
    if (f == 1) {
        const size_t blocks = (slab + 255) / 256;
        FFNO_LAUNCH(export_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, vel,
                    vort + off, vx + off, vy + off, slab);
        return status();
    }
    const int R = rows(m);
    FFNO_LAUNCH(export_coarsen_kernel, dim3(slices(m), B), dim3(256), sizeof(float) * (size_t)(2 * R + 1) * m, (hipStream_t)stream,
                vel, vort + off, vx + off, vy + off, X, Y, m, f, R, len_x / (float)m, len_y / (float)m);
    return status();
}

extern "C" int ffno_energy_spectrum(const float* u_h, const float* v_h, float* E, int n_img, int m, void* stream) {
    using namespace ffno::pred_export;
    if (!u_h || !v_h || !E || n_img <= 0 || m <= 0) return FFNO_EINVAL;
    if (m % 8 || m < kSpecMinM || m > kSpecMaxM) return FFNO_EUNSUPPORTED;
    const double m2 = (double)m * m;
    FFNO_LAUNCH(energy_spectrum_kernel, dim3((unsigned)n_img), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float2*>(u_h), reinterpret_cast<const float2*>(v_h), E, m, (float)(1.0 / (2.0 * m2 * m2)));
    return status();
}
