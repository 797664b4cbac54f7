// Fused feed-forward of the WIDE F-FNO block (widths 96 .. 256) for a pass that saves nothing: one launch in place of the pair
//     ffno_bgemm (relu, bias):  h = relu(S W1^T + b1)   [P, H] to HBM          (feedforward.py:13-19)
//     ffno_bgemm (bias, resid): out = h W2^T + b2 (+ resid)                     (grid_2d.py:169)
//     out[p][c] = ( sum_j relu( sum_i S[p][i] W1[j][i] + b1[j] ) W2[c][j] ) + b2[c]  (+ resid[p][c])
// The hidden image h never leaves the CU.  Same instruction (v_mfma_f32_32x32x2_f32) and same summation order as bgemm.hip, so the
// result is the pair's, bit for bit: every hidden unit is one accumulator over i = 0 .. C-1 in ascending pairs, then + b1, max(., 0);
// every output element is one accumulator over j = 0 .. H-1 in ascending pairs, living across the chunks, then + b2, then + resid.
//   workgroup  4 waves, 128 pixel rows; wave w owns rows 32 w .. 32 w + 31 for BOTH products, so h is exchanged inside a wave only
//   registers  the wave's S rows as the A operand of GEMM 1 (C / 2 per lane, loaded once), the [32 x C] output tile (C / 2 per
//              lane), one [32 x 32] hidden tile, and the NEXT chunk's weights on their way from global memory to LDS (C / 4 per lane)
//   H chunks   32 hidden units: W1 rows h0 .. h0 + 31 ([32 x C]) and W2 columns h0 .. h0 + 31 ([C x 32]) in one of two LDS buffers.
//              Per chunk: request chunk n + 1 (global -> registers), GEMM 1 (C / 2 MFMAs), bias + ReLU, h through the wave's own
//              LDS tile (D layout -> A layout), GEMM 2 (C / 2 MFMAs), registers -> the other buffer, ONE workgroup barrier.  The
//              global loads are in flight during all the chunk's MFMAs.
//   LDS image  of an operand X[row][k] (k contiguous in memory): img[half][row][m] = X[row][2 m + half], row pitch K / 2 + 2 floats.
//              A lane of half `half` reads its operands of two consecutive MFMAs with one 8-byte read; the pitch is 2 (mod 4), so
//              the 32 lanes of a half hit 32 distinct bank pairs: conflict-free.
// An ordinary launch, grid = row tiles; no atomics: two runs are bit-identical.
#include "ffno_device.h"
#include "ffno.h"

namespace ffno {

constexpr int kFfRows = 128;               // pixel rows per workgroup
constexpr int kFfHC = 32;                  // hidden units per chunk
constexpr int kFfPH = kFfHC / 2 + 2;       // plane row pitch of the images with K = 32 (h, the W2 chunk)
constexpr int kFfAhead = 4;                // GEMM 1: 8-byte B reads in flight ahead of the MFMA pair that consumes them

template <int CT>
struct FfLds {      // in floats
    static constexpr int C = 32 * CT;
    static constexpr int P1 = C / 2 + 2;              // plane row pitch of the images with K = C (the W1 chunk, the S rows)
    static constexpr int W1 = 2 * 32 * P1;
    static constexpr int W2 = 2 * C * kFfPH;
    static constexpr int BUF = W1 + W2;               // one weight chunk
    static constexpr int HW = 2 * 32 * kFfPH;         // one wave's hidden tile
    static constexpr int TOTAL = 2 * BUF + 4 * HW;
    static_assert(4 * W1 <= 2 * BUF, "the four S tiles are staged through the weight buffers");
};

struct FfArgs {
    ffno_bgemm_ff_desc d;
    int nchunk;
};

// chunk n of both weights and of b1: global -> registers
template <int CT>
__device__ __forceinline__ void ff_fetch(const ffno_bgemm_ff_desc& d, int n, float4* w1r, float4* w2r, float& b1r) {
    constexpr int C = 32 * CT;
    const int tid = threadIdx.x, h0 = n * kFfHC;
    const float* w1 = d.W1 + (int64_t)h0 * C;         // rows h0 .. h0 + 31 of [H][C]: 32 C contiguous floats
    FFNO_UNROLL
    for (int u = 0; u < CT; ++u) w1r[u] = *reinterpret_cast<const float4*>(w1 + 4 * (tid + 256 * u));
    FFNO_UNROLL
    for (int u = 0; u < CT; ++u) {
        const int idx = tid + 256 * u, c = idx >> 3, q = idx & 7;
        w2r[u] = *reinterpret_cast<const float4*>(d.W2 + (int64_t)c * d.H + h0 + 4 * q);
    }
    b1r = d.b1[h0 + (tid & 31)];
}

// four consecutive k of one row -> the two planes of an image (plane size `plane`, at row * pitch + m)
__device__ __forceinline__ void ff_put4(float* img, int plane, int at, float4 v) {
    *reinterpret_cast<float2*>(img + at) = make_float2(v.x, v.z);
    *reinterpret_cast<float2*>(img + plane + at) = make_float2(v.y, v.w);
}

// registers -> the LDS images of a weight chunk
template <int CT>
__device__ __forceinline__ void ff_stash(float* buf, const float4* w1r, const float4* w2r) {
    using L = FfLds<CT>;
    constexpr int C = L::C;
    const int tid = threadIdx.x;
    FFNO_UNROLL
    for (int u = 0; u < CT; ++u) {
        const int idx = tid + 256 * u, r = idx / (C / 4), q = idx % (C / 4);
        ff_put4(buf, 32 * L::P1, r * L::P1 + 2 * q, w1r[u]);
    }
    FFNO_UNROLL
    for (int u = 0; u < CT; ++u) {
        const int idx = tid + 256 * u, c = idx >> 3, q = idx & 7;
        ff_put4(buf + L::W1, C * kFfPH, c * kFfPH + 2 * q, w2r[u]);
    }
}

template <int CT>
__global__ __launch_bounds__(256) void bgemm_ff_kernel(FfArgs g) {
    using L = FfLds<CT>;
    constexpr int C = L::C, P1 = L::P1, PH = kFfPH;
    FFNO_DYN_SMEM(smem_raw);
    float* lds = reinterpret_cast<float*>(smem_raw);
    const ffno_bgemm_ff_desc& d = g.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * kFfRows + wave * 32;

    float4 w1r[CT], w2r[CT];
    float b1r;
    ff_fetch<CT>(d, 0, w1r, w2r, b1r);

    // the wave's 32 rows of S (zero past row P - 1) -> its A operand of GEMM 1: lane (j, half) holds S[row j][2 m + half]
    float sreg[C / 2];
    {
        float* img = lds + wave * L::W1;
        FFNO_UNROLL
        for (int u = 0; u < 4 * CT; ++u) {
            const int idx = lane + 64 * u, r = idx / (C / 4), q = idx % (C / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < d.P) v = *reinterpret_cast<const float4*>(d.S + (row0 + r) * d.s_rs + 4 * q);
            ff_put4(img, 32 * P1, r * P1 + 2 * q, v);
        }
        plat::wave_sync();
        const float* sp = img + half * 32 * P1 + j * P1;
        FFNO_UNROLL
        for (int mm = 0; mm < C / 4; ++mm) {
            const float2 v = *reinterpret_cast<const float2*>(sp + 2 * mm);
            sreg[2 * mm] = v.x, sreg[2 * mm + 1] = v.y;
        }
    }
    __syncthreads();      // (the S tiles lie in the weight buffers)
    ff_stash<CT>(lds, w1r, w2r);
    __syncthreads();

    f32x16 acc[CT];
    FFNO_UNROLL
    for (int ct = 0; ct < CT; ++ct) acc[ct] = zero16();
    float* himg = lds + 2 * L::BUF + wave * L::HW;

    FFNO_NOUNROLL
    for (int n = 0; n < g.nchunk; ++n) {
        const float* buf = lds + (n & 1) * L::BUF;
        const float b1v = b1r;
        if (n + 1 < g.nchunk) ff_fetch<CT>(d, n + 1, w1r, w2r, b1r);      // in flight during this chunk's MFMAs

        // GEMM 1: hidden tile [32 rows x 32 units], K = C
        f32x16 hacc = zero16();
        const float* w1p = buf + half * 32 * P1 + j * P1;
        // (one wave per SIMD: the B reads run kFfAhead MFMA pairs ahead of their use, or every read's latency is exposed)
        float2 bq[kFfAhead];
        FFNO_UNROLL
        for (int mm = 0; mm < kFfAhead; ++mm) bq[mm] = *reinterpret_cast<const float2*>(w1p + 2 * mm);
        FFNO_UNROLL
        for (int mm = 0; mm < C / 4; ++mm) {
            const float2 b = bq[mm % kFfAhead];
            if (mm + kFfAhead < C / 4) {
                bq[mm % kFfAhead] = *reinterpret_cast<const float2*>(w1p + 2 * (mm + kFfAhead));
                FFNO_SCHED_PIN_DSREAD();
            }
            hacc = mfma32(sreg[2 * mm], b.x, hacc);
            hacc = mfma32(sreg[2 * mm + 1], b.y, hacc);
        }
        // + b1, ReLU (bg_store's order); D layout (lane: unit j, rows drow) -> the A image of GEMM 2
        plat::wave_sync();      // (the wave has read the previous chunk's tile)
        FFNO_UNROLL
        for (int r = 0; r < 16; ++r) himg[(j & 1) * 32 * PH + drow(r, half) * PH + (j >> 1)] = fmaxf(hacc[r] + b1v, 0.f);
        plat::wave_sync();

        // GEMM 2: the [32 x C] output tile += h [32 x 32] . W2[:, h0 .. h0 + 31]^T
        const float* ap = himg + half * 32 * PH + j * PH;
        const float* bp = buf + L::W1 + half * C * PH + j * PH;
        FFNO_UNROLL
        for (int mm = 0; mm < kFfHC / 4; ++mm) {
            const float2 a = *reinterpret_cast<const float2*>(ap + 2 * mm);
            FFNO_UNROLL
            for (int ct = 0; ct < CT; ++ct) {
                const float2 b = *reinterpret_cast<const float2*>(bp + ct * 32 * PH + 2 * mm);
                acc[ct] = mfma32(a.x, b.x, acc[ct]);
                acc[ct] = mfma32(a.y, b.y, acc[ct]);
            }
        }
        if (n + 1 < g.nchunk) ff_stash<CT>(lds + ((n + 1) & 1) * L::BUF, w1r, w2r);      // (last read before the previous barrier)
        __syncthreads();
    }

    FFNO_UNROLL
    for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 32 + j;
        const float b2v = d.b2[c];
        FFNO_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int64_t p = row0 + drow(r, half);
            if (p >= d.P) continue;
            float v = acc[ct][r] + b2v;
            if (d.resid) v += d.resid[p * d.resid_rs + c];
            d.out[p * d.out_rs + c] = v;
        }
    }
}

static inline bool ff_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// [a, a + na) and [b, b + nb) floats share an address
static inline bool ff_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 4 * (uintptr_t)nb && b0 < a0 + 4 * (uintptr_t)na;
}

static inline int ff_check(const ffno_bgemm_ff_desc* d) {
    if (!d || !d->S || !d->W1 || !d->b1 || !d->W2 || !d->b2 || !d->out || d->P < 1) return FFNO_EINVAL;
    if (d->C % 32 || d->C < 96 || d->C > 256 || d->H % kFfHC || d->H < kFfHC || d->H > 1024) return FFNO_EUNSUPPORTED;
    const int64_t strides[3] = {d->s_rs, d->out_rs, d->resid ? d->resid_rs : d->out_rs};
    for (int64_t rs : strides) {
        if (rs < d->C || rs % 4 || rs >= (1LL << 31) || d->P > (1LL << 38) / rs) return FFNO_EUNSUPPORTED;
    }
    if (!ff_aligned16(d->S) || !ff_aligned16(d->W1) || !ff_aligned16(d->W2) || !ff_aligned16(d->out) || !ff_aligned16(d->resid))
        return FFNO_EUNSUPPORTED;
    if ((d->P + kFfRows - 1) / kFfRows >= (1LL << 31)) return FFNO_EUNSUPPORTED;
    const int64_t no = (d->P - 1) * d->out_rs + d->C;
    if (ff_overlap(d->out, no, d->S, (d->P - 1) * d->s_rs + d->C)) return FFNO_EUNSUPPORTED;
    if (d->resid && ff_overlap(d->out, no, d->resid, (d->P - 1) * d->resid_rs + d->C)) return FFNO_EUNSUPPORTED;
    return FFNO_OK;
}

template <int CT>
static int ff_launch(const FfArgs& g, hipStream_t st) {
    const size_t smem = sizeof(float) * (size_t)FfLds<CT>::TOTAL;
    const int e = allow_dynamic_lds(bgemm_ff_kernel<CT>, smem);
    if (e) return e;
    FFNO_LAUNCH(bgemm_ff_kernel<CT>, dim3((unsigned)((g.d.P + kFfRows - 1) / kFfRows)), dim3(256), smem, st, g);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? FFNO_OK : (int)err;
}

}  // namespace ffno

using namespace ffno;

extern "C" int ffno_bgemm_ff_supported(const ffno_bgemm_ff_desc* d) { return ff_check(d) == FFNO_OK ? 1 : 0; }

extern "C" int ffno_bgemm_ff(const ffno_bgemm_ff_desc* d, void* stream) {
    const int rc = ff_check(d);
    if (rc) return rc;
    FfArgs g;
    g.d = *d;
    g.nchunk = d->H / kFfHC;
    hipStream_t st = (hipStream_t)stream;
    switch (d->C / 32) {
        case 3: return ff_launch<3>(g, st);
        case 4: return ff_launch<4>(g, st);
        case 5: return ff_launch<5>(g, st);
        case 6: return ff_launch<6>(g, st);
        case 7: return ff_launch<7>(g, st);
        default: return ff_launch<8>(g, st);
    }
}
