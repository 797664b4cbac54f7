// IPhi, the coordinate deformation network of the elasticity F-FNO (reference fourierflow/modules/iphi.py:27-58), for
// P = B N points and width w, H = 4 w:
//     xd   = [x0, x1, atan2(x1 - c, x0 - c), |x - (c, c)|]                       c = 1e-4
//     f    = [fc_code(code_b) | fc0(xd) | sin(B_k xd_d) | cos(B_k xd_d)]           B_k = fl32(pi) 2^k, k < w / 4, index d (w/4) + k
//     a1 = tanh(fc1 f), a2 = tanh(fc2 a1), a3 = tanh(fc3 a2),  xi = x + x * fc4(a3)
// Forward: ONE launch.  A workgroup owns 32 points (two workgroups share a CU's LDS); their activations [32][H] stay in LDS from
// the features to fc4, the three H x H layers run on v_mfma_f32_32x32x2_f32 (exact fp32) with the weights streamed through LDS
// 32 input columns at a time -- the next chunk's global loads are in flight while the current one feeds the matrix cores.
// For training the four layer inputs f, a1, a2, a3 are also written to `acts` ([4][P][H]).
// Backward: the same tile walks the chain in reverse (dz3 -> dz2 -> dz1 -> df, weights read untransposed), then the three
// H x H weight gradients are one batched MFMA launch over point slices, the thin layers (fc4, fc0) a VALU launch over 64-point
// slices, fc_code's per-sample sums a third, and one reduction sums the slices in a fixed order: deterministic, no atomics.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace iphi {

static constexpr int kPts = 32;                    // points per workgroup (one MFMA row tile)
static constexpr int kKC = 32;                     // rows of a weight chunk in LDS
static constexpr int kWT = 64;                     // weight-gradient tile (64 x 64 outputs per workgroup)
static constexpr int kMaxB = 8;                    // samples whose fc_code output a workgroup keeps in LDS
static constexpr int kCode = FFNO_IPHI_CODE_DIM;   // 42
static constexpr float kCenter = 1e-4f;
static constexpr float kPiF = 3.14159274101257324f;   // fl32(pi): what np.pi * float32 tensor gives

typedef ffno_iphi_params Params;

// B_k v as ONE rounded fp32 product (the reference multiplies two fp32 tensors; a contracted product would feed sin an
// argument that differs by up to half an ulp -- at B_15 = pi 2^15 that is visible in the sine)
__device__ __forceinline__ float freq_arg(int k, float v) {
#pragma clang fp contract(off)
    const float bk = kPiF * (float)(1 << k);      // exact scaling
    const float p = bk * v;
    return p;
}

__device__ __forceinline__ float4 features(float2 x) {
    const float dx = x.x - kCenter, dy = x.y - kCenter;
    return make_float4(x.x, x.y, atan2f(dy, dx), sqrtf(dx * dx + dy * dy));
}

// acc[u] = act[32][H] (LDS, row stride H + 1) times one H x H weight matrix; wave w owns the column tiles w + 4 u.
// TRANS = false: out[q][o] = sum_i act[q][i] W[o][i] (forward); TRANS = true: out[q][i] = sum_o act[q][o] W[o][i] (backward
// data).  The weights pass through registers on their way to LDS, so the loads of chunk k + 1 overlap the MFMAs of chunk k.
// Ends with a barrier: the caller may overwrite act.
template <int H, bool TRANS>
__device__ __forceinline__ void tile_gemm(const float* __restrict__ W, const float* act, float* wsm, f32x16 (&acc)[(H + 127) / 128]) {
    constexpr int LD = H + 1, NT = H / 32, NU = (NT + 3) / 4, NP = kKC * H / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    float pre[NP];
    auto fetch = [&](int k0) {
        FFNO_UNROLL
        for (int t = 0; t < NP; ++t) {
            const int e = tid + 256 * t;
            if (TRANS) {
                const int k = e / H, n = e - k * H;
                pre[t] = W[(long)(k0 + k) * H + n];
            } else {
                const int n = e / kKC, k = e - n * kKC;
                pre[t] = W[(long)n * H + k0 + k];
            }
        }
    };
    FFNO_UNROLL
    for (int u = 0; u < NU; ++u) acc[u] = zero16();
    fetch(0);
    FFNO_NOUNROLL
    for (int k0 = 0; k0 < H; k0 += kKC) {
        __syncthreads();   // act is complete / the previous chunk is consumed
        FFNO_UNROLL
        for (int t = 0; t < NP; ++t) {
            const int e = tid + 256 * t;
            if (TRANS) {
                const int k = e / H, n = e - k * H;
                wsm[k * LD + n] = pre[t];
            } else {
                const int n = e / kKC, k = e - n * kKC;
                wsm[k * LD + n] = pre[t];
            }
        }
        __syncthreads();
        if (k0 + kKC < H) fetch(k0 + kKC);
        _Pragma("unroll 4")
        for (int kk = 0; kk < kKC; kk += 2) {
            const float a = act[j * LD + k0 + kk + half];
            FFNO_UNROLL
            for (int u = 0; u < NU; ++u)      // (every wave owns NU full tiles once H >= 128)
                if (NT % 4 == 0 || wave + 4 * u < NT) acc[u] = mfma32(a, wsm[(kk + half) * LD + (wave + 4 * u) * 32 + j], acc[u]);
        }
    }
    __syncthreads();
}

template <int H>
__global__ __launch_bounds__(256) FFNO_WAVES_PER_SIMD(2) void iphi_fwd_kernel(Params p, const float2* __restrict__ x, const float* __restrict__ code,
                                                       float2* __restrict__ xi, float4* __restrict__ feat,
                                                       float* __restrict__ acts, int N, long P) {
    FFNO_DYN_SMEM(smem);
    constexpr int W = H / 4, NF = W / 4, LD = H + 1, NT = H / 32, NU = (NT + 3) / 4;
    float* act = reinterpret_cast<float*>(smem);     // [32][H + 1]
    float* wsm = act + kPts * LD;                    // [32][H + 1]
    float* fs = wsm + kKC * LD;                      // [32][4]
    float* cds = fs + 4 * kPts;                      // [kMaxB][W]: fc_code(code_b) of the samples this tile touches
    const int tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * kPts;
    const long plast = p0 + kPts - 1 < P ? p0 + kPts - 1 : P - 1;
    const int b0 = (int)(p0 / N), nb = (int)(plast / N) - b0 + 1;
    if (nb <= kMaxB) {
        FFNO_NOUNROLL
        for (int e = tid; e < nb * W; e += 256) {
            const int bb = e / W, jj = e - bb * W;
            const float* c = code + (long)(b0 + bb) * kCode;
            const float* w = p.code_w + jj * kCode;
            float v = p.code_b[jj];
            for (int k = 0; k < kCode; ++k) v = fmaf(w[k], c[k], v);
            cds[e] = v;
        }
    }
    if (tid < kPts) {
        const long pp = p0 + tid;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pp < P) {
            f = features(x[pp]);
            if (feat) feat[pp] = f;
        }
        fs[tid * 4] = f.x, fs[tid * 4 + 1] = f.y, fs[tid * 4 + 2] = f.z, fs[tid * 4 + 3] = f.w;
    }
    __syncthreads();
    FFNO_NOUNROLL
    for (int e = tid; e < kPts * H; e += 256) {
        const int q = e / H, j = e - q * H;
        const long pp = p0 + q;
        float v = 0.f;
        if (pp < P) {
            const float* f = fs + q * 4;
            if (j < W) {
                if (nb <= kMaxB) {
                    v = cds[((int)(pp / N) - b0) * W + j];
                } else {      // the tile touches more than kMaxB samples: every point evaluates its own (same order: same bits)
                    const float* c = code + (pp / N) * kCode;
                    const float* w = p.code_w + j * kCode;
                    v = p.code_b[j];
                    for (int k = 0; k < kCode; ++k) v = fmaf(w[k], c[k], v);
                }
            } else if (j < 2 * W) {
                const int jj = j - W;
                v = p.fc0_b[jj];
                for (int d = 0; d < 4; ++d) v = fmaf(p.fc0_w[jj * 4 + d], f[d], v);
            } else {
                const bool is_sin = j < 3 * W;
                const int jj = j - (is_sin ? 2 : 3) * W;
                const float arg = freq_arg(jj % NF, f[jj / NF]);
                v = is_sin ? sinf(arg) : cosf(arg);
            }
            if (acts) acts[pp * H + j] = v;
        }
        act[q * LD + j] = v;
    }
    const int lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    f32x16 acc[NU];
    FFNO_NOUNROLL
    for (int l = 0; l < 3; ++l) {
        const float* Wl = l == 0 ? p.fc1_w : (l == 1 ? p.fc2_w : p.fc3_w);
        const float* bl = l == 0 ? p.fc1_b : (l == 1 ? p.fc2_b : p.fc3_b);
        tile_gemm<H, false>(Wl, act, wsm, acc);
        FFNO_UNROLL
        for (int u = 0; u < NU; ++u) {
            if (NT % 4 != 0 && wave + 4 * u >= NT) continue;
            const int col = (wave + 4 * u) * 32 + j;
            const float b = bl[col];
            FFNO_UNROLL
            for (int r = 0; r < 16; ++r) {
                const int row = drow(r, half);
                const float v = tanhf(acc[u][r] + b);
                act[row * LD + col] = v;
                if (acts && p0 + row < P) acts[((long)(l + 1) * P + p0 + row) * H + col] = v;
            }
        }
    }
    __syncthreads();
    if (tid < 2 * kPts) {
        const int q = tid >> 1, d = tid & 1;
        const long pp = p0 + q;
        if (pp < P) {
            float s = p.fc4_b[d];
            for (int k = 0; k < H; ++k) s = fmaf(act[q * LD + k], p.fc4_w[d * H + k], s);
            const float xv = fs[q * 4 + d];
            reinterpret_cast<float*>(xi)[pp * 2 + d] = fmaf(xv, s, xv);
        }
    }
}

// dz[l - 1] = d loss / d (pre-activation of fc_l), l = 1..3, [3][P][H];  dfa[P][2 w] = the gradient of f's first two blocks
// (fc_code's and fc0's outputs; the sin / cos block has no parameters)
template <int H>
__global__ __launch_bounds__(256) FFNO_WAVES_PER_SIMD(2) void iphi_bwd_data_kernel(Params p, const float2* __restrict__ x, const float2* __restrict__ dxi,
                                                            const float* __restrict__ acts, float* __restrict__ dz,
                                                            float* __restrict__ dfa, long P) {
    FFNO_DYN_SMEM(smem);
    constexpr int W = H / 4, LD = H + 1, NT = H / 32, NU = (NT + 3) / 4;
    float* G = reinterpret_cast<float*>(smem);
    float* wsm = G + kPts * LD;
    float* g4 = wsm + kKC * LD;                      // [32][2]
    const int tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * kPts;
    if (tid < kPts) {
        const long pp = p0 + tid;
        float2 g = make_float2(0.f, 0.f);
        if (pp < P) {
            const float2 xv = x[pp], d = dxi[pp];
            g = make_float2(d.x * xv.x, d.y * xv.y);
        }
        g4[tid * 2] = g.x, g4[tid * 2 + 1] = g.y;
    }
    __syncthreads();
    FFNO_NOUNROLL
    for (int e = tid; e < kPts * H; e += 256) {
        const int q = e / H, j = e - q * H;
        const long pp = p0 + q;
        float v = 0.f;
        if (pp < P) {
            const float a = acts[(3 * P + pp) * H + j];
            v = fmaf(g4[q * 2], p.fc4_w[j], g4[q * 2 + 1] * p.fc4_w[H + j]) * (1.f - a * a);
            dz[(2 * P + pp) * H + j] = v;
        }
        G[q * LD + j] = v;
    }
    const int lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    f32x16 acc[NU];
    FFNO_NOUNROLL
    for (int l = 2; l >= 0; --l) {      // through fc_{l + 1}: l = 2, 1 give dz_l, l = 0 gives df
        const float* Wl = l == 2 ? p.fc3_w : (l == 1 ? p.fc2_w : p.fc1_w);
        tile_gemm<H, true>(Wl, G, wsm, acc);
        FFNO_UNROLL
        for (int u = 0; u < NU; ++u) {
            if (NT % 4 != 0 && wave + 4 * u >= NT) continue;
            const int col = (wave + 4 * u) * 32 + j;
            FFNO_UNROLL
            for (int r = 0; r < 16; ++r) {
                const int row = drow(r, half);
                const long pp = p0 + row;
                if (l > 0) {
                    float v = 0.f;
                    if (pp < P) {
                        const float a = acts[((long)l * P + pp) * H + col];
                        v = acc[u][r] * (1.f - a * a);
                        dz[((long)(l - 1) * P + pp) * H + col] = v;
                    }
                    G[row * LD + col] = v;
                } else if (col < 2 * W && pp < P) {
                    dfa[pp * (2 * W) + col] = acc[u][r];
                }
            }
        }
    }
}

// dW_l[o][i] = sum_p dz_l[p][o] a_{l-1}[p][i], db_l[o] = sum_p dz_l[p][o] over the point slice blockIdx.y, layer blockIdx.z:
// partial[slice][layer][H H + H]
__global__ __launch_bounds__(256) void iphi_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ acts,
                                                         float* __restrict__ partial, int H, long P, int chunk) {
    __shared__ float Zs[kKC][kWT + 1];
    __shared__ float As[kKC][kWT + 1];
    const int tiles_n = H / kWT, layer = blockIdx.z;
    const int m0 = (blockIdx.x / tiles_n) * kWT, n0 = (blockIdx.x % tiles_n) * kWT;
    const long kbeg = (long)blockIdx.y * chunk, kend = kbeg + chunk < P ? kbeg + chunk : P;
    const float* Z = dz + (long)layer * P * H;
    const float* A = acts + (long)layer * P * H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, j = lane & 31, half = lane >> 5;
    f32x16 acc = zero16();
    float rs = 0.f;
    for (long k0 = kbeg; k0 < kend; k0 += kKC) {
        FFNO_UNROLL
        for (int t = 0; t < kKC * kWT / 256; ++t) {
            const int e = tid + 256 * t, k = e / kWT, c = e - k * kWT;
            const long pp = k0 + k;
            Zs[k][c] = pp < kend ? Z[pp * H + m0 + c] : 0.f;
            As[k][c] = pp < kend ? A[pp * H + n0 + c] : 0.f;
        }
        __syncthreads();
        FFNO_UNROLL
        for (int kk = 0; kk < kKC; kk += 2) acc = mfma32(Zs[kk + half][wr * 32 + j], As[kk + half][wc * 32 + j], acc);
        if (n0 == 0 && tid < kWT)
            for (int k = 0; k < kKC; ++k) rs += Zs[k][tid];
        __syncthreads();
    }
    float* part = partial + ((long)blockIdx.y * 3 + layer) * ((long)H * H + H);
    FFNO_UNROLL
    for (int r = 0; r < 16; ++r) part[(long)(m0 + wr * 32 + drow(r, half)) * H + n0 + wc * 32 + j] = acc[r];
    if (n0 == 0 && tid < kWT) part[(long)H * H + m0 + tid] = rs;
}

// the thin layers over the point slice blockIdx.x: small[slice] = { dW4 [2][H], db4 [2], dW0 [w][4], db0 [w] }
__global__ __launch_bounds__(256) void iphi_small_kernel(const float2* __restrict__ x, const float2* __restrict__ dxi,
                                                         const float* __restrict__ feat, const float* __restrict__ acts,
                                                         const float* __restrict__ dfa, float* __restrict__ small, int H, long P,
                                                         int chunk) {
    const int W = H / 4, nsm = 2 * H + 2 + 5 * W;
    const long kbeg = (long)blockIdx.x * chunk, kend = kbeg + chunk < P ? kbeg + chunk : P;
    const float* g = reinterpret_cast<const float*>(dxi);
    const float* xv = reinterpret_cast<const float*>(x);
    const float* a3 = acts + 3 * P * H;
    for (int e = threadIdx.x; e < nsm; e += 256) {
        float s = 0.f;
        if (e < 2 * H) {
            const int d = e / H, jj = e - d * H;
            for (long pp = kbeg; pp < kend; ++pp) s = fmaf(g[pp * 2 + d] * xv[pp * 2 + d], a3[pp * H + jj], s);
        } else if (e < 2 * H + 2) {
            const int d = e - 2 * H;
            for (long pp = kbeg; pp < kend; ++pp) s += g[pp * 2 + d] * xv[pp * 2 + d];
        } else if (e < 2 * H + 2 + 4 * W) {
            const int t = e - (2 * H + 2), jj = t >> 2, d = t & 3;
            for (long pp = kbeg; pp < kend; ++pp) s = fmaf(dfa[pp * (2 * W) + W + jj], feat[pp * 4 + d], s);
        } else {
            const int jj = e - (2 * H + 2 + 4 * W);
            for (long pp = kbeg; pp < kend; ++pp) s += dfa[pp * (2 * W) + W + jj];
        }
        small[(long)blockIdx.x * nsm + e] = s;
    }
}

// per sample: dcd[b][j] = sum_n dfa[b, n][j] (fc_code's output is shared by the sample's points), dcode[b] = dcd[b] Wc
__global__ __launch_bounds__(256) void iphi_code_kernel(const float* __restrict__ dfa, const float* __restrict__ code_w,
                                                        float* __restrict__ dcd, float* __restrict__ dcode, int W, int N) {
    __shared__ float red[4][64];
    const int b = blockIdx.x, j = threadIdx.x & 63, grp = threadIdx.x >> 6;
    float s = 0.f;
    if (j < W)
        for (int n = grp; n < N; n += 4) s += dfa[((long)b * N + n) * (2 * W) + j];
    red[grp][j] = s;
    __syncthreads();
    if (threadIdx.x < W) {
        s = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
        red[0][j] = s;
        dcd[b * W + j] = s;
    }
    __syncthreads();
    if (threadIdx.x < kCode) {
        float t = 0.f;
        for (int jj = 0; jj < W; ++jj) t = fmaf(red[0][jj], code_w[jj * kCode + threadIdx.x], t);
        dcode[b * kCode + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(256) void iphi_reduce_kernel(Params g, const float* __restrict__ partial, const float* __restrict__ small,
                                                          const float* __restrict__ dcd, const float* __restrict__ code, int H, int B,
                                                          int nsplit, int nsmall) {
    const int W = H / 4, nsm = 2 * H + 2 + 5 * W;
    const long nl = (long)H * H + H, n_big = 3 * nl, n_code = (long)W * kCode + W;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_big + nsm + n_code) return;
    float s = 0.f;
    if (e < n_big) {
        const int l = (int)(e / nl);
        const long r = e - l * nl;
        for (int sp = 0; sp < nsplit; ++sp) s += partial[((long)sp * 3 + l) * nl + r];
        float* dW = l == 0 ? g.fc1_w : (l == 1 ? g.fc2_w : g.fc3_w);
        float* db = l == 0 ? g.fc1_b : (l == 1 ? g.fc2_b : g.fc3_b);
        if (r < (long)H * H) dW[r] = s;
        else db[r - (long)H * H] = s;
    } else if (e < n_big + nsm) {
        const int r = (int)(e - n_big);
        for (int sp = 0; sp < nsmall; ++sp) s += small[(long)sp * nsm + r];
        if (r < 2 * H) g.fc4_w[r] = s;
        else if (r < 2 * H + 2) g.fc4_b[r - 2 * H] = s;
        else if (r < 2 * H + 2 + 4 * W) g.fc0_w[r - (2 * H + 2)] = s;
        else g.fc0_b[r - (2 * H + 2 + 4 * W)] = s;
    } else {
        const int r = (int)(e - n_big - nsm);
        if (r < W * kCode) {
            const int jj = r / kCode, k = r - jj * kCode;
            for (int b = 0; b < B; ++b) s = fmaf(dcd[b * W + jj], code[b * kCode + k], s);
            g.code_w[r] = s;
        } else {
            const int jj = r - W * kCode;
            for (int b = 0; b < B; ++b) s += dcd[b * W + jj];
            g.code_b[jj] = s;
        }
    }
}

static inline size_t lds_bytes(int H) { return sizeof(float) * ((size_t)(kPts + kKC) * (H + 1) + 4 * kPts + (size_t)kMaxB * (H / 4)); }
static constexpr int kSmallChunk = 64;             // points per slice of the thin-layer gradients
static inline int nsmall_of(long P) { return (int)((P + kSmallChunk - 1) / kSmallChunk); }
static inline int nsplit_of(long P) { return (int)(P < 1024 ? 1 : (P + 1023) / 1024 > 64 ? 64 : (P + 1023) / 1024); }
static inline int chunk_of(long P) {
    const int ns = nsplit_of(P);
    return (int)(((P + ns - 1) / ns + kKC - 1) / kKC * kKC);
}
static inline bool params_ok(const Params* p) {
    return p && p->fc0_w && p->fc0_b && p->code_w && p->code_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && p->fc3_w &&
           p->fc3_b && p->fc4_w && p->fc4_b;
}
static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

template <int H>
static int launch_fwd(const Params& p, const float* x, const float* code, float* xi, float* feat, float* acts, int N, long P,
                      hipStream_t st) {
    const size_t lds = lds_bytes(H);
    const int e = allow_dynamic_lds(iphi_fwd_kernel<H>, lds);
    if (e) return e;
    FFNO_LAUNCH(iphi_fwd_kernel<H>, dim3((unsigned)((P + kPts - 1) / kPts)), dim3(256), lds, st, p,
                reinterpret_cast<const float2*>(x), code, reinterpret_cast<float2*>(xi), reinterpret_cast<float4*>(feat), acts, N, P);
    return status();
}
template <int H>
static int launch_bwd_data(const Params& p, const float* x, const float* dxi, const float* acts, float* dz, float* dfa, long P,
                           hipStream_t st) {
    const size_t lds = lds_bytes(H);
    const int e = allow_dynamic_lds(iphi_bwd_data_kernel<H>, lds);
    if (e) return e;
    FFNO_LAUNCH(iphi_bwd_data_kernel<H>, dim3((unsigned)((P + kPts - 1) / kPts)), dim3(256), lds, st, p,
                reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(dxi), acts, dz, dfa, P);
    return status();
}

}  // namespace iphi
}  // namespace ffno

extern "C" int ffno_iphi_supported(int width) { return width == 16 || width == 32 || width == 64; }

extern "C" size_t ffno_iphi_bwd_ws_floats(int B, int N, int width) {
    using namespace ffno::iphi;
    if (B <= 0 || N <= 0 || !ffno_iphi_supported(width)) return 0;
    const long P = (long)B * N;
    const size_t H = 4 * (size_t)width, ns = (size_t)nsplit_of(P);
    return 3 * (size_t)P * H + (size_t)P * 2 * width + ns * 3 * (H * H + H) +
           (size_t)nsmall_of(P) * (2 * H + 2 + 5 * (size_t)width) +
           (size_t)B * width;
}

extern "C" int ffno_iphi_fwd(const ffno_iphi_params* params, const float* x, const float* code, float* xi, float* feat,
                             float* acts, int B, int N, int width, void* stream) {
    using namespace ffno::iphi;
    if (!params_ok(params) || !x || !code || !xi || B <= 0 || N <= 0) return FFNO_EINVAL;
    if (!ffno_iphi_supported(width) || (long)B * N * 4 * width >= (1L << 31)) return FFNO_EUNSUPPORTED;
    const long P = (long)B * N;
    hipStream_t st = (hipStream_t)stream;
    switch (width) {
        case 16: return launch_fwd<64>(*params, x, code, xi, feat, acts, N, P, st);
        case 32: return launch_fwd<128>(*params, x, code, xi, feat, acts, N, P, st);
        default: return launch_fwd<256>(*params, x, code, xi, feat, acts, N, P, st);
    }
}

extern "C" int ffno_iphi_bwd(const ffno_iphi_params* params, const ffno_iphi_params* grads, const float* x, const float* code,
                             const float* feat, const float* acts, const float* dxi, float* dcode, float* ws, int B, int N,
                             int width, void* stream) {
    using namespace ffno::iphi;
    if (!params_ok(params) || !params_ok(grads) || !x || !code || !feat || !acts || !dxi || !dcode || !ws || B <= 0 || N <= 0)
        return FFNO_EINVAL;
    if (!ffno_iphi_supported(width) || (long)B * N * 4 * width >= (1L << 31)) return FFNO_EUNSUPPORTED;
    const long P = (long)B * N;
    const int H = 4 * width, ns = nsplit_of(P), chunk = chunk_of(P), nsm = 2 * H + 2 + 5 * width;
    float* dz = ws;
    float* dfa = dz + 3 * P * H;
    float* partial = dfa + P * 2 * width;
    float* small = partial + (long)ns * 3 * ((long)H * H + H);
    float* dcd = small + (long)nsmall_of(P) * nsm;
    hipStream_t st = (hipStream_t)stream;
    int rc = width == 16   ? launch_bwd_data<64>(*params, x, dxi, acts, dz, dfa, P, st)
             : width == 32 ? launch_bwd_data<128>(*params, x, dxi, acts, dz, dfa, P, st)
                           : launch_bwd_data<256>(*params, x, dxi, acts, dz, dfa, P, st);
    if (rc) return rc;
    FFNO_LAUNCH(iphi_wgrad_kernel, dim3((H / kWT) * (H / kWT), ns, 3), dim3(256), 0, st, dz, acts, partial, H, P, chunk);
    if ((rc = status())) return rc;
    FFNO_LAUNCH(iphi_small_kernel, dim3(nsmall_of(P)), dim3(256), 0, st, reinterpret_cast<const float2*>(x),
                reinterpret_cast<const float2*>(dxi), feat, acts, dfa, small, H, P, kSmallChunk);
    if ((rc = status())) return rc;
    FFNO_LAUNCH(iphi_code_kernel, dim3(B), dim3(256), 0, st, dfa, params->code_w, dcd, dcode, width, N);
    if ((rc = status())) return rc;
    const long total = 3 * ((long)H * H + H) + nsm + (long)width * kCode + width;
    FFNO_LAUNCH(iphi_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *grads, partial, small, dcd, code, H, B,
                ns, nsmall_of(P));
    return status();
}
