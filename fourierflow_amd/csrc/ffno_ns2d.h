// One Crank-Nicolson step of the pseudo-spectral 2-D Navier-Stokes solver behind `generate navier-stokes` (reference
// fourierflow/builders/synthetic/ns_2d.py:126-175), on torch.fft.rfft2 HALF spectra [B][N][N/2+1][2]:
//     ffno_ns2d_derivs     w_h -> the spectra of q = psi_y, v = -psi_x, w_x, w_y        (ns_2d.py:128-156, one read of w_h)
//     (one batched irfft2 of the four)
//     ffno_ns2d_advect     q w_x + v w_y on the four real fields                         (ns_2d.py:159, the product)
//     (one rfft2)
//     ffno_ns2d_cn_update  dealias, force, Crank-Nicolson update of w_h in place         (ns_2d.py:163, 173-175)
// The time-varying random force (ns_2d.py:167-170, 203-237) is a sum of 3 cycles plane waves with fixed amplitudes and one common
// phase phi = t_scaling t: in a half spectrum it has 4 cycles non-zero bins per sample, each a fixed amplitude rotated by
// e^{+-i phi}.  ffno_ns2d_cn_update_harmonic is the update with those bins computed from amp[B][cycles][6] and (cos phi, sin phi)
// -- no force field, no force transform, no f_h stream; ffno_ns2d_harmonic_force writes the field itself for the snapshots.
// Wavenumbers come from the indices: row r is k_x = r (r < N/2) or r - N, column c is k_y = c; no tables.  The reference
// transforms the FULL spectrum and keeps `.real`, which drops the derivative along an axis at that axis' Nyquist bin (the
// products i k w there are anti-Hermitian); irfft2 would keep the row k_x = -N/2, so derivs writes zeros there.
// All three stream: one thread moves 16 bytes (two complex bins / four reals) per tensor and trip of a grid-stride loop, no LDS,
// no atomics.  N is a power of two, so a pair of bins never straddles two samples and row / sample indices are shifts and masks
// after one division by N/2+1.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace ns2d {

static constexpr float kTwoPi = 6.28318530717958647692f, kFourPiSq = 39.4784176043574344753f;
static constexpr unsigned kMaxBlocks = 8192;

// bin e (counted over all samples) -> row r, column c; next() steps to bin e + 1
struct Bin {
    int r, c;
    unsigned row;      // b N + r
    __device__ __forceinline__ Bin(unsigned e, int N, int Nh) {
        row = e / (unsigned)Nh;
        c = (int)(e - row * (unsigned)Nh);
        r = (int)(row & (unsigned)(N - 1));
    }
    __device__ __forceinline__ void next(int N, int Nh) {
        if (++c == Nh) c = 0, ++row, r = (r + 1) & (N - 1);
    }
    __device__ __forceinline__ int kx(int N) const { return r < N / 2 ? r : r - N; }
    __device__ __forceinline__ float lap(int N) const {
        const int k = kx(N), k2 = k * k + c * c;
        return k2 ? kFourPiSq * (float)k2 : 1.f;
    }
};

// (q, v, w_x, w_y) of one bin w = (re, im)
__device__ __forceinline__ void derivs_bin(float re, float im, const Bin& b, int N, float2& q, float2& v, float2& wx, float2& wy) {
    const float lap = b.lap(N);
    const float pr = re / lap, pi = im / lap;                       // psi_h = w_h / lap
    const float sx = b.r == N / 2 ? 0.f : kTwoPi * (float)b.kx(N);   // the Nyquist row of d/dx, the Nyquist column of d/dy: zero
    const float sy = b.c == N / 2 ? 0.f : kTwoPi * (float)b.c;
    q = make_float2(-sy * pi, sy * pr);
    v = make_float2(sx * pi, -sx * pr);
    wx = make_float2(-sx * im, sx * re);
    wy = make_float2(-sy * im, sy * re);
}

__global__ __launch_bounds__(256) void ns2d_derivs_kernel(const float4* __restrict__ w, float4* __restrict__ out, unsigned pairs,
                                                          int N) {
    const int Nh = N / 2 + 1;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u) {
        const float4 a = w[p];
        Bin b(2u * p, N, Nh);
        float2 q0, v0, x0, y0, q1, v1, x1, y1;
        derivs_bin(a.x, a.y, b, N, q0, v0, x0, y0);
        b.next(N, Nh);
        derivs_bin(a.z, a.w, b, N, q1, v1, x1, y1);
        out[p] = make_float4(q0.x, q0.y, q1.x, q1.y);
        out[(size_t)pairs + p] = make_float4(v0.x, v0.y, v1.x, v1.y);
        out[2 * (size_t)pairs + p] = make_float4(x0.x, x0.y, x1.x, x1.y);
        out[3 * (size_t)pairs + p] = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
}

__global__ __launch_bounds__(256) void ns2d_advect_kernel(const float4* __restrict__ f, float4* __restrict__ out, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 q = f[i], v = f[n4 + i], wx = f[2 * n4 + i], wy = f[3 * n4 + i];
        out[i] = make_float4(fmaf(q.x, wx.x, v.x * wy.x), fmaf(q.y, wx.y, v.y * wy.y), fmaf(q.z, wx.z, v.z * wy.z),
                             fmaf(q.w, wx.w, v.w * wy.w));
    }
}

// one bin of the update: w <- (-dt F dealias + dt f + (1 - factor) w) / (1 + factor), factor = 0.5 dt nu lap
__device__ __forceinline__ float2 cn_bin(float2 w, float2 F, float2 f, const Bin& b, int N, float dt, float half_dt_nu) {
    const int ak = b.kx(N) < 0 ? -b.kx(N) : b.kx(N);
    const float keep = (3 * ak <= N && 3 * b.c <= N) ? 1.f : 0.f;      // |k| <= (2/3)(N/2): exact for a power-of-two N
    const float factor = half_dt_nu * b.lap(N);
    const float d = 1.f + factor, m = 1.f - factor;
    return make_float2((-dt * (F.x * keep) + dt * f.x + m * w.x) / d, (-dt * (F.y * keep) + dt * f.y + m * w.y) / d);
}

// FMODE 0: no force, 1: one force spectrum for every sample, 2: one per sample
template <int FMODE>
__global__ __launch_bounds__(256) void ns2d_cn_kernel(float4* __restrict__ w, const float4* __restrict__ F, const float4* __restrict__ fh,
                                                      const float* __restrict__ visc, float dt, unsigned pairs, int N, int lgN) {
    const int Nh = N / 2 + 1;
    const unsigned sample_pairs = (unsigned)N * (unsigned)Nh / 2u;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u) {
        const float4 a = w[p], g = F[p];
        Bin b(2u * p, N, Nh);
        const unsigned s = b.row >> lgN;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (FMODE == 1) f = fh[p - s * sample_pairs];
        if (FMODE == 2) f = fh[p];
        const float hdn = 0.5f * dt * visc[s];
        const float2 r0 = cn_bin(make_float2(a.x, a.y), make_float2(g.x, g.y), make_float2(f.x, f.y), b, N, dt, hdn);
        b.next(N, Nh);
        const float2 r1 = cn_bin(make_float2(a.z, a.w), make_float2(g.z, g.w), make_float2(f.z, f.w), b, N, dt, hdn);
        w[p] = make_float4(r0.x, r0.y, r1.x, r1.y);
    }
}

// The harmonic force  scaling sum_p a1 sin(k x + phi) + a2 cos(k x + phi) + a3 sin(k y + phi) + a4 cos(k y + phi)
// + a5 sin(k (x + y) + phi) + a6 cos(k (x + y) + phi),  k = 2 pi p, p = 1 .. cycles < N/2, in one bin of the unnormalised half
// spectrum; a = amp of this sample [cycles][6], h = scaling N^2 / 2, e = cp + i sp.  Non-zero are (p, 0): h (a2 - i a1) e,
// (N - p, 0): h (a2 + i a1) conj(e), (0, p): h (a4 - i a3) e and (p, p): h (a6 - i a5) e.
__device__ __forceinline__ float2 harmonic_bin(const float* __restrict__ a, const Bin& b, int N, int cycles, float h, float cp,
                                               float sp) {
    float re, im, s = sp;
    if (b.c == 0) {
        if (b.r >= 1 && b.r <= cycles) a += 6 * (b.r - 1), re = a[1], im = -a[0];
        else if (b.r >= N - cycles) a += 6 * (N - b.r - 1), re = a[1], im = a[0], s = -sp;
        else return make_float2(0.f, 0.f);
    } else if (b.c <= cycles) {
        a += 6 * (b.c - 1);
        if (b.r == 0) re = a[3], im = -a[2];
        else if (b.r == b.c) re = a[5], im = -a[4];
        else return make_float2(0.f, 0.f);
    } else {
        return make_float2(0.f, 0.f);
    }
    return make_float2(h * (re * cp - im * s), h * (re * s + im * cp));
}

// ns2d_cn_kernel with the force of a bin from harmonic_bin: a kernel of its own, so that the three modes above stay as they are
__global__ __launch_bounds__(256) void ns2d_cn_harmonic_kernel(float4* __restrict__ w, const float4* __restrict__ F,
                                                               const float* __restrict__ amp, const float* __restrict__ visc, float dt,
                                                               float h, float cp, float sp, int cycles, unsigned pairs, int N, int lgN) {
    const int Nh = N / 2 + 1;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u) {
        const float4 a = w[p], g = F[p];
        Bin b(2u * p, N, Nh);
        const unsigned s = b.row >> lgN;
        const float* as = amp + (size_t)s * 6u * (unsigned)cycles;
        const float hdn = 0.5f * dt * visc[s];
        const float2 r0 = cn_bin(make_float2(a.x, a.y), make_float2(g.x, g.y), harmonic_bin(as, b, N, cycles, h, cp, sp), b, N, dt, hdn);
        b.next(N, Nh);
        const float2 r1 = cn_bin(make_float2(a.z, a.w), make_float2(g.z, g.w), harmonic_bin(as, b, N, cycles, h, cp, sp), b, N, dt, hdn);
        w[p] = make_float4(r0.x, r0.y, r1.x, r1.y);
    }
}

// one grid point of the harmonic force before the factor `scaling`: the grid angles 2 pi (p i mod N) / N are reduced exactly in
// integers (N a power of two) and the phase comes in by the angle-sum formulas, so the error depends on neither p nor phi
__device__ __forceinline__ float harmonic_point(const float* __restrict__ a, int i, int j, int N, int cycles, float cp, float sp) {
    const float two_over_N = 2.f / (float)N;
    float f = 0.f;
    for (int p = 1; p <= cycles; ++p, a += 6) {
        const int m[3] = {(p * i) & (N - 1), (p * j) & (N - 1), (p * (i + j)) & (N - 1)};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float s, c;
            plat::sincos_pi(two_over_N * (float)m[d], s, c);
            f = fmaf(a[2 * d], fmaf(s, cp, c * sp), f);             // sin(theta + phi)
            f = fmaf(a[2 * d + 1], fmaf(c, cp, -(s * sp)), f);      // cos(theta + phi)
        }
    }
    return f;
}

__global__ __launch_bounds__(256) void ns2d_harmonic_force_kernel(const float* __restrict__ amp, float4* __restrict__ f, size_t n4,
                                                                  float scaling, float cp, float sp, int cycles, int N, int lgN) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (size_t)gridDim.x * 256) {
        const size_t e = 4 * q;                                    // N is a multiple of 4: the four points share a row
        const int j = (int)(e & (size_t)(N - 1)), i = (int)((e >> lgN) & (size_t)(N - 1));
        const float* a = amp + (e >> (2 * lgN)) * 6u * (unsigned)cycles;
        f[q] = make_float4(scaling * harmonic_point(a, i, j, N, cycles, cp, sp), scaling * harmonic_point(a, i, j + 1, N, cycles, cp, sp),
                           scaling * harmonic_point(a, i, j + 2, N, cycles, cp, sp), scaling * harmonic_point(a, i, j + 3, N, cycles, cp, sp));
    }
}

static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static inline int log2_of(int N) {
    int l = 0;
    while ((1 << l) < N) ++l;
    return l;
}
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
static inline unsigned blocks_for(size_t items) {
    const size_t b = (items + 255) / 256;
    return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}
// bins of B half spectra, or 0 where the 32-bit bin index of the kernels would not hold them
static inline size_t bins_of(int B, int N) {
    const size_t bins = (size_t)B * N * (N / 2 + 1);
    return bins < ((size_t)1 << 31) ? bins : 0;
}

}  // namespace ns2d
}  // namespace ffno

extern "C" int ffno_ns2d_supported(int N) { return N >= 8 && N <= 512 && (N & (N - 1)) == 0; }

extern "C" int ffno_ns2d_derivs(const float* w_h, float* out4, int B, int N, void* stream) {
    using namespace ffno::ns2d;
    if (!w_h || !out4 || B <= 0 || N <= 0 || !aligned16(w_h) || !aligned16(out4)) return FFNO_EINVAL;
    const size_t bins = ffno_ns2d_supported(N) ? bins_of(B, N) : 0;
    if (!bins) return FFNO_EUNSUPPORTED;
    FFNO_LAUNCH(ns2d_derivs_kernel, dim3(blocks_for(bins / 2)), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float4*>(w_h), reinterpret_cast<float4*>(out4), (unsigned)(bins / 2), N);
    return status();
}

extern "C" int ffno_ns2d_advect(const float* fields4, float* out, size_t n, void* stream) {
    using namespace ffno::ns2d;
    if (!fields4 || !out || n == 0 || n % 4 || !aligned16(fields4) || !aligned16(out)) return FFNO_EINVAL;
    FFNO_LAUNCH(ns2d_advect_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float4*>(fields4), reinterpret_cast<float4*>(out), n / 4);
    return status();
}

extern "C" int ffno_ns2d_cn_update(float* w_h, const float* F_h, const float* f_h, const float* visc, float delta_t, int f_batched,
                                   int B, int N, void* stream) {
    using namespace ffno::ns2d;
    if (!w_h || !F_h || !visc || B <= 0 || N <= 0 || !aligned16(w_h) || !aligned16(F_h) || !aligned16(f_h)) return FFNO_EINVAL;
    const size_t bins = ffno_ns2d_supported(N) ? bins_of(B, N) : 0;
    if (!bins) return FFNO_EUNSUPPORTED;
    const unsigned pairs = (unsigned)(bins / 2);
    const dim3 grid(blocks_for(pairs));
    hipStream_t st = (hipStream_t)stream;
    float4* w = reinterpret_cast<float4*>(w_h);
    const float4 *F = reinterpret_cast<const float4*>(F_h), *f = reinterpret_cast<const float4*>(f_h);
    if (!f_h) FFNO_LAUNCH(ns2d_cn_kernel<0>, grid, dim3(256), 0, st, w, F, f, visc, delta_t, pairs, N, log2_of(N));
    else if (!f_batched) FFNO_LAUNCH(ns2d_cn_kernel<1>, grid, dim3(256), 0, st, w, F, f, visc, delta_t, pairs, N, log2_of(N));
    else FFNO_LAUNCH(ns2d_cn_kernel<2>, grid, dim3(256), 0, st, w, F, f, visc, delta_t, pairs, N, log2_of(N));
    return status();
}

extern "C" int ffno_ns2d_cn_update_harmonic(float* w_h, const float* F_h, const float* amp, const float* visc, float delta_t,
                                            float scaling, float cos_phi, float sin_phi, int cycles, int B, int N, void* stream) {
    using namespace ffno::ns2d;
    if (!w_h || !F_h || !amp || !visc || B <= 0 || N <= 0 || !aligned16(w_h) || !aligned16(F_h) || !aligned4(amp) || !aligned4(visc))
        return FFNO_EINVAL;
    const size_t bins = ffno_ns2d_supported(N) ? bins_of(B, N) : 0;
    if (!bins || cycles < 1 || cycles >= N / 2) return FFNO_EUNSUPPORTED;
    const unsigned pairs = (unsigned)(bins / 2);
    FFNO_LAUNCH(ns2d_cn_harmonic_kernel, dim3(blocks_for(pairs)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(w_h),
                reinterpret_cast<const float4*>(F_h), amp, visc, delta_t, scaling * (0.5f * (float)N * (float)N), cos_phi, sin_phi, cycles,
                pairs, N, log2_of(N));
    return status();
}

extern "C" int ffno_ns2d_harmonic_force(const float* amp, float* f, float scaling, float cos_phi, float sin_phi, int cycles, int B, int N,
                                        void* stream) {
    using namespace ffno::ns2d;
    if (!amp || !f || B <= 0 || N <= 0 || !aligned4(amp) || !aligned16(f)) return FFNO_EINVAL;
    if (!ffno_ns2d_supported(N) || !bins_of(B, N) || cycles < 1 || cycles >= N / 2) return FFNO_EUNSUPPORTED;
    const size_t n4 = (size_t)B * N * N / 4;
    FFNO_LAUNCH(ns2d_harmonic_force_kernel, dim3(blocks_for(n4)), dim3(256), 0, (hipStream_t)stream, amp, reinterpret_cast<float4*>(f),
                n4, scaling, cos_phi, sin_phi, cycles, N, log2_of(N));
    return status();
}
