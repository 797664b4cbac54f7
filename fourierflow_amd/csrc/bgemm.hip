// Batched strided fp32 GEMM on the fp32 matrix cores: the kernel family of the WIDE F-FNO block (widths 96 .. 256).
//
// The tuned kernels (spectral_x3*, ffx, ff, spectral, pointwise lift / head, infer) are specialised for 32 or 64 channels.  The
// reference block is width-agnostic (fourierflow/modules/factorized_fno/grid_2d.py:103-152); for the widths the tuned kernels do not
// take, engine_wide.py composes the whole block -- lift, per-axis truncated DFTs, per-mode complex channel mix, feed-forward, head,
// and all their adjoints and weight gradients -- from ONE kernel:
//     D[g1][g0][m][n] = epilogue( alpha * sum_k A[g1][g0][m][k] * B[g1][g0][k][n] )
//     epilogue(v):  v += bias[n];  v = max(v, 0) (relu);  v = gate[m][n] > 0 ? v : 0;  v += resid[m][n];  v += D[m][n] (accumulate)
// A, B, D are read / written through 64-bit (row, column, batch level 0, batch level 1) strides: no operand is ever transposed or
// copied in HBM, a batch stride of 0 shares an operand.  gate / resid are addressed like D.  v_mfma_f32_32x32x2_f32 is a k-ordered
// fmaf chain, so every tile variant gives the same bits: exact fp32.
//   tiles     block = 4 waves; (waves along m) x (waves along n) x (32 x 32 MFMA tiles per wave along m, n):
//             128 x 128 (2 x 2 waves, 2 x 2 tiles), 64 x 64 (2 x 2, 1 x 1), 32 x 128 (1 x 4: M <= 32, the rows of a DFT matrix),
//             128 x 32 (4 x 1: N <= 32, the head).  K is staged through LDS in chunks of 32; tiles and chunks are zero padded.
//   staging   16-byte global loads along whichever of an operand's two dimensions has unit stride when base and strides are
//             16-byte aligned, else 4-byte loads walking the dimension of the smaller stride.  D is stored one float per lane, a
//             32-lane row of the MFMA tile = 128 contiguous bytes when d_cs = 1.
//   split-K   weight gradients (K = pixels): slices of at most 4096 rows into a caller-provided partial buffer, folded in slice
//             order by a second launch that applies the epilogue.  No atomics: two runs are bit-identical.  The same for the
//             column sum of the bias gradients.
#include <algorithm>

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {

constexpr int kBK = 32;              // K chunk
constexpr int kBgSlice = 4096;       // split-K: most rows per slice
constexpr int kBgColRows = 1024;     // column sum: rows per slice

struct BgArgs {
    ffno_bgemm_desc d;
    int a_mode, b_mode;      // staging: 0 scalar / column fastest, 1 scalar / row fastest, 2 16-byte along columns, 3 16-byte along rows
    int tiles_m, tiles_n;
    int kslice;              // rows of K per blockIdx.y
    float* partial;          // split-K: [slice][g][M][N] raw sums; else NULL
};

// tile T[R][CC] (zero padded) of src -> lds[r * (CC + 1) + c]
template <int R, int CC>
__device__ __forceinline__ void bg_stage(float* lds, const float* __restrict__ src, int64_t rs, int64_t cs, int r0, int c0, int rmax,
                                         int cmax, int mode) {
    const int tid = threadIdx.x;
    if (mode == 2) {
        constexpr int CV = CC / 4;
        FFNO_UNROLL
        for (int e = tid; e < R * CV; e += 256) {
            const int r = e / CV, c = (e % CV) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < rmax && c0 + c < cmax) {
                const float* p = src + (int64_t)(r0 + r) * rs + (c0 + c);
                if (c0 + c + 3 < cmax) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    v.x = p[0];
                    if (c0 + c + 1 < cmax) v.y = p[1];
                    if (c0 + c + 2 < cmax) v.z = p[2];
                }
            }
            float* q = lds + r * (CC + 1) + c;
            q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        }
    } else if (mode == 3) {
        constexpr int RV = R / 4;
        FFNO_UNROLL
        for (int e = tid; e < RV * CC; e += 256) {
            const int r = (e % RV) * 4, c = e / RV;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < rmax && c0 + c < cmax) {
                const float* p = src + (int64_t)(c0 + c) * cs + (r0 + r);
                if (r0 + r + 3 < rmax) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    v.x = p[0];
                    if (r0 + r + 1 < rmax) v.y = p[1];
                    if (r0 + r + 2 < rmax) v.z = p[2];
                }
            }
            float* q = lds + r * (CC + 1) + c;
            q[0] = v.x, q[CC + 1] = v.y, q[2 * (CC + 1)] = v.z, q[3 * (CC + 1)] = v.w;
        }
    } else {
        for (int e = tid; e < R * CC; e += 256) {
            const int r = mode ? e % R : e / CC, c = mode ? e / R : e % CC;
            float v = 0.f;
            if (r0 + r < rmax && c0 + c < cmax) v = src[(int64_t)(r0 + r) * rs + (int64_t)(c0 + c) * cs];
            lds[r * (CC + 1) + c] = v;
        }
    }
}

__device__ __forceinline__ void bg_store(const ffno_bgemm_desc& d, int64_t idx, int n, float v) {
    v *= d.alpha;
    if (d.bias) v += d.bias[n];
    if (d.relu) v = fmaxf(v, 0.f);
    if (d.gate) v = d.gate[idx] > 0.f ? v : 0.f;
    if (d.resid) v += d.resid[idx];
    if (d.accumulate) v += d.D[idx];
    d.D[idx] = v;
}

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void bgemm_kernel(BgArgs g) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    static_assert(WM * WN == 4, "four waves");
    __shared__ float As[BM * (kBK + 1)];
    __shared__ float Bs[kBK * (BN + 1)];
    const ffno_bgemm_desc& d = g.d;
    const int tiles = g.tiles_m * g.tiles_n;
    const int64_t gi = blockIdx.x / tiles;
    const int t = blockIdx.x % tiles;
    const int m0 = (t / g.tiles_n) * BM, n0 = (t % g.tiles_n) * BN;
    const int64_t g0 = gi % d.G0, g1 = gi / d.G0;
    const float* A = d.A + g0 * d.a_g0 + g1 * d.a_g1;
    const float* B = d.B + g0 * d.b_g0 + g1 * d.b_g1;
    const int kbeg = blockIdx.y * g.kslice, kend = min(d.K, kbeg + g.kslice);

    f32x16 acc[TM][TN];
    FFNO_UNROLL
    for (int i = 0; i < TM; ++i) {
        FFNO_UNROLL
        for (int j = 0; j < TN; ++j) acc[i][j] = zero16();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave / WN, wc = wave % WN;
    const int j = lane & 31, half = lane >> 5;
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
        bg_stage<BM, kBK>(As, A, d.a_rs, d.a_cs, m0, k0, d.M, kend, g.a_mode);
        bg_stage<kBK, BN>(Bs, B, d.b_rs, d.b_cs, k0, n0, kend, d.N, g.b_mode);
        __syncthreads();
        FFNO_UNROLL
        for (int kk = 0; kk < kBK; kk += 2) {
            float a[TM], b[TN];
            FFNO_UNROLL
            for (int i = 0; i < TM; ++i) a[i] = As[((wr * TM + i) * 32 + j) * (kBK + 1) + kk + half];
            FFNO_UNROLL
            for (int i = 0; i < TN; ++i) b[i] = Bs[(kk + half) * (BN + 1) + (wc * TN + i) * 32 + j];
            FFNO_UNROLL
            for (int im = 0; im < TM; ++im) {
                FFNO_UNROLL
                for (int in = 0; in < TN; ++in) acc[im][in] = mfma32(a[im], b[in], acc[im][in]);
            }
        }
        __syncthreads();
    }
    FFNO_UNROLL
    for (int im = 0; im < TM; ++im) {
        FFNO_UNROLL
        for (int in = 0; in < TN; ++in) {
            const int n = n0 + (wc * TN + in) * 32 + j;
            if (n >= d.N) continue;
            FFNO_UNROLL
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wr * TM + im) * 32 + drow(r, half);
                if (m >= d.M) continue;
                if (g.partial) {
                    const int64_t G = (int64_t)d.G0 * d.G1;
                    g.partial[(((int64_t)blockIdx.y * G + gi) * d.M + m) * d.N + n] = acc[im][in][r];
                } else {
                    bg_store(d, g0 * d.d_g0 + g1 * d.d_g1 + (int64_t)m * d.d_rs + (int64_t)n * d.d_cs, n, acc[im][in][r]);
                }
            }
        }
    }
}

// D = epilogue(alpha * sum over slices, in slice order)
__global__ __launch_bounds__(256) void bgemm_fold_kernel(ffno_bgemm_desc d, const float* __restrict__ partial, int nslice) {
    const int64_t per = (int64_t)d.M * d.N, G = (int64_t)d.G0 * d.G1;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per * G) return;
    float s = 0.f;
    for (int sl = 0; sl < nslice; ++sl) s += partial[(int64_t)sl * per * G + e];
    const int64_t gi = e / per;
    const int m = (int)((e % per) / d.N), n = (int)(e % d.N);
    const int64_t g0 = gi % d.G0, g1 = gi / d.G0;
    bg_store(d, g0 * d.d_g0 + g1 * d.d_g1 + (int64_t)m * d.d_rs + (int64_t)n * d.d_cs, n, s);
}

// column sums: block (column chunk of 64, slice): 4 row groups x 64 columns, each thread walks its rows in order, the groups are
// added in order; partial[slice][N]
__global__ __launch_bounds__(256) void bgemm_colsum_kernel(const float* __restrict__ X, int64_t rs, int64_t P, int N,
                                                           float* __restrict__ partial) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
    const int64_t pbeg = (int64_t)blockIdx.y * kBgColRows, pend = min(P, pbeg + kBgColRows);
    float s = 0.f;
    if (n < N)
        for (int64_t p = pbeg + rg; p < pend; p += 4) s += X[p * rs + n];
    red[rg][c] = s;
    __syncthreads();
    if (rg == 0 && n < N) partial[(int64_t)blockIdx.y * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}
__global__ __launch_bounds__(256) void bgemm_colsum_fold_kernel(const float* __restrict__ partial, float* out, int N, int nslice,
                                                                int accumulate) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int sl = 0; sl < nslice; ++sl) s += partial[(int64_t)sl * N + n];
    out[n] = accumulate ? out[n] + s : s;
}

// fourier_weight [C][C][K][2] (in, out, mode, re / im) -> Wb[k][2C][2C] = [[Wr, Wi], [-Wi, Wr]] (rows: in, columns: out)
__global__ __launch_bounds__(256) void bgemm_pack_fw_kernel(const float* __restrict__ w, float* __restrict__ Wb, int C, int K) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n2 = 2 * (int64_t)C;
    if (e >= (int64_t)K * n2 * n2) return;
    const int col = (int)(e % n2), row = (int)((e / n2) % n2), k = (int)(e / (n2 * n2));
    const int i = row % C, o = col % C, ri = row / C, ci = col / C;
    const float* p = w + (((int64_t)i * C + o) * K + k) * 2;
    Wb[e] = ri == ci ? p[0] : (ri == 0 ? p[1] : -p[1]);
}
// G[k][2C][2C] = [[G11, G12], [G21, G22]] -> dw[i][o][k] = (G11 + G22, G12 - G21)
__global__ __launch_bounds__(256) void bgemm_fold_fw_kernel(const float* __restrict__ G, float* dw, int C, int K, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)C * C * K) return;
    const int k = (int)(e % K), o = (int)((e / K) % C), i = (int)(e / ((int64_t)K * C));
    const int64_t n2 = 2 * (int64_t)C;
    const float* g = G + (int64_t)k * n2 * n2;
    const float re = g[i * n2 + o] + g[(i + C) * n2 + o + C];
    const float im = g[i * n2 + o + C] - g[(i + C) * n2 + o];
    float* q = dw + 2 * e;
    q[0] = accumulate ? q[0] + re : re;
    q[1] = accumulate ? q[1] + im : im;
}

static inline int bg_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

// how an operand tile [rows][cols] is staged (BgArgs::a_mode)
static inline int bg_mode(const float* p, int64_t rs, int64_t cs, int64_t s0, int64_t s1) {
    const bool base = (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && s0 % 4 == 0 && s1 % 4 == 0;
    if (cs == 1 && base && rs % 4 == 0) return 2;
    if (rs == 1 && base && cs % 4 == 0) return 3;
    const int64_t ar = rs < 0 ? -rs : rs, ac = cs < 0 ? -cs : cs;
    return ac <= ar ? 0 : 1;
}

enum { BG_T128 = 0, BG_T64, BG_TM32, BG_TN32 };
static inline int bg_variant(int M, int N) {
    if (M <= 32) return BG_TM32;
    if (N <= 32) return BG_TN32;
    if (M <= 64 || N <= 64) return BG_T64;
    return BG_T128;
}
static inline void bg_tile(int variant, int& BM, int& BN) {
    BM = variant == BG_T128 ? 128 : variant == BG_T64 ? 64 : variant == BG_TM32 ? 32 : 128;
    BN = variant == BG_T128 ? 128 : variant == BG_T64 ? 64 : variant == BG_TM32 ? 128 : 32;
}

static inline int bg_check(const ffno_bgemm_desc* d) {
    if (!d || !d->A || !d->B || !d->D) return FFNO_EINVAL;
    if (d->M < 1 || d->N < 1 || d->K < 1 || d->G0 < 1 || d->G1 < 1) return FFNO_EINVAL;
    // every output element has its own address: no zero stride on D, and a batch level that is there moves D
    if (d->d_rs == 0 || d->d_cs == 0 || (d->G0 > 1 && d->d_g0 == 0) || (d->G1 > 1 && d->d_g1 == 0)) return FFNO_EUNSUPPORTED;
    int BM, BN;
    bg_tile(bg_variant(d->M, d->N), BM, BN);
    const int64_t blocks = (int64_t)((d->M + BM - 1) / BM) * ((d->N + BN - 1) / BN) * d->G0 * d->G1;
    if (blocks >= (1LL << 31) || (int64_t)d->M * d->N * d->G0 * d->G1 >= (1LL << 38)) return FFNO_EUNSUPPORTED;
    return FFNO_OK;
}

// slices of K: at most kBgSlice rows, halved (down to 512) while the launch has fewer than 256 workgroups
static inline int bg_kslice(const ffno_bgemm_desc* d) {
    int BM, BN;
    bg_tile(bg_variant(d->M, d->N), BM, BN);
    const int64_t blocks = (int64_t)((d->M + BM - 1) / BM) * ((d->N + BN - 1) / BN) * d->G0 * d->G1;
    int ks = kBgSlice;
    while (ks > 512 && blocks * ((d->K + ks - 1) / ks) < 256) ks /= 2;
    return ks;
}

static int bg_launch(const ffno_bgemm_desc* d, float* partial, int kslice, int nslice, hipStream_t st) {
    BgArgs g;
    g.d = *d;
    g.a_mode = bg_mode(d->A, d->a_rs, d->a_cs, d->a_g0, d->a_g1);
    g.b_mode = bg_mode(d->B, d->b_rs, d->b_cs, d->b_g0, d->b_g1);
    const int variant = bg_variant(d->M, d->N);
    int BM, BN;
    bg_tile(variant, BM, BN);
    g.tiles_m = (d->M + BM - 1) / BM;
    g.tiles_n = (d->N + BN - 1) / BN;
    g.kslice = kslice;
    g.partial = partial;
    const dim3 grid((unsigned)((int64_t)g.tiles_m * g.tiles_n * d->G0 * d->G1), nslice), block(256);
    switch (variant) {
        case BG_T128: FFNO_LAUNCH((bgemm_kernel<2, 2, 2, 2>), grid, block, 0, st, g); break;
        case BG_T64: FFNO_LAUNCH((bgemm_kernel<2, 2, 1, 1>), grid, block, 0, st, g); break;
        case BG_TM32: FFNO_LAUNCH((bgemm_kernel<1, 4, 1, 1>), grid, block, 0, st, g); break;
        default: FFNO_LAUNCH((bgemm_kernel<4, 1, 1, 1>), grid, block, 0, st, g); break;
    }
    return bg_status();
}

}  // namespace ffno

using namespace ffno;

extern "C" int ffno_bgemm_supported(const ffno_bgemm_desc* d) { return bg_check(d) == FFNO_OK ? 1 : 0; }

extern "C" int ffno_bgemm(const ffno_bgemm_desc* d, void* stream) {
    const int rc = bg_check(d);
    if (rc) return rc;
    return bg_launch(d, nullptr, d->K, 1, (hipStream_t)stream);
}

extern "C" int ffno_bgemm_splitk_slices(const ffno_bgemm_desc* d) {
    if (bg_check(d)) return 0;
    const int ks = bg_kslice(d);
    return (d->K + ks - 1) / ks;
}
extern "C" size_t ffno_bgemm_splitk_ws_floats(const ffno_bgemm_desc* d) {
    return (size_t)ffno_bgemm_splitk_slices(d) * (size_t)(bg_check(d) ? 0 : (int64_t)d->M * d->N * d->G0 * d->G1);
}

extern "C" int ffno_bgemm_splitk(const ffno_bgemm_desc* d, float* partial, void* stream) {
    const int rc = bg_check(d);
    if (rc) return rc;
    if (!partial) return FFNO_EINVAL;
    const int ks = bg_kslice(d), nslice = (d->K + ks - 1) / ks;
    if (nslice > 65535) return FFNO_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int rl = bg_launch(d, partial, ks, nslice, st);
    if (rl) return rl;
    const int64_t n = (int64_t)d->M * d->N * d->G0 * d->G1;
    FFNO_LAUNCH(bgemm_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *d, (const float*)partial, nslice);
    return bg_status();
}

extern "C" size_t ffno_bgemm_colsum_ws_floats(long P, int N) {
    return P <= 0 || N <= 0 ? 0 : (size_t)((P + kBgColRows - 1) / kBgColRows) * (size_t)N;
}
extern "C" int ffno_bgemm_colsum(const float* X, long row_stride, long P, int N, float* partial, float* out, int accumulate,
                                 void* stream) {
    if (!X || !partial || !out || P <= 0 || N <= 0) return FFNO_EINVAL;
    const long nslice = (P + kBgColRows - 1) / kBgColRows;
    if (nslice > 65535) return FFNO_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    FFNO_LAUNCH(bgemm_colsum_kernel, dim3((N + 63) / 64, (unsigned)nslice), dim3(256), 0, st, X, (int64_t)row_stride, (int64_t)P, N,
                partial);
    const int rc = bg_status();
    if (rc) return rc;
    FFNO_LAUNCH(bgemm_colsum_fold_kernel, dim3((N + 255) / 256), dim3(256), 0, st, (const float*)partial, out, N, (int)nslice,
                accumulate);
    return bg_status();
}

extern "C" int ffno_bgemm_pack_fw(const float* w, float* Wb, int C, int K, void* stream) {
    if (!w || !Wb || C <= 0 || K <= 0) return FFNO_EINVAL;
    const int64_t n = 4 * (int64_t)C * C * K;
    if (n >= (1LL << 38)) return FFNO_EUNSUPPORTED;
    FFNO_LAUNCH(bgemm_pack_fw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Wb, C, K);
    return bg_status();
}
extern "C" int ffno_bgemm_fold_fw(const float* G, float* dw, int C, int K, int accumulate, void* stream) {
    if (!G || !dw || C <= 0 || K <= 0) return FFNO_EINVAL;
    const int64_t n = (int64_t)C * C * K;
    if (n >= (1LL << 38)) return FFNO_EUNSUPPORTED;
    FFNO_LAUNCH(bgemm_fold_fw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, dw, C, K, accumulate);
    return bg_status();
}
