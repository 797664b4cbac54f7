// Zero padding and cropping of channels-last fp32 activations: what the WIDE mesh operators (FNOFactorizedMesh2D / Mesh3D at widths
// 96 .. 256, engine_wide.py) put between the dense lift / head GEMMs and the layers on the padded grid.
//
// The reference pads the lifted features once, `F.pad(x, [0, p, ...])` at the END of every spatial axis (mesh_2d.py:150,
// mesh_3d.py:165), and crops the last backcast, `b[..., :-p, :]` (mesh_2d.py:158, mesh_3d.py:173).  The two maps are each other's
// adjoint, so the backward pass uses the same pair the other way round.
//     ffno_pad_embed   dense [B][s_0]..[s_{D-1}][C]  ->  padded [B][s_0 + p_0]..[s_{D-1} + p_{D-1}][C]; EVERY element of the destination
//                      is written, the pad region with 0.0f (the destination may be a reused buffer)
//     ffno_pad_crop    padded -> dense
// One kernel serves both.  It walks the elements of the DESTINATION as float4 (C % 4 == 0, 16-byte loads and stores) in a
// grid-stride loop and keeps the destination index as a mixed-radix counter (last axis x channels, the two axes before it, and
// everything outside folded into the top digit): the divisions that split an index into coordinates run once per thread, before
// the loop, and every turn adds the launch's stride -- split into the same digits on the host -- with carries.  The source offset
// is three 64-bit multiply-adds on the digits.  Memory-bound; at most 2048 blocks of 256 threads.  No LDS, no atomics.
#include <algorithm>

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {

constexpr int kPadBlock = 256;
constexpr int kPadMaxBlocks = 2048;      // 256 CUs x 8 blocks; larger tensors go round the grid-stride loop

struct PadArgs {
    int64_t total;      // float4 elements of the destination
    int it[3];          // destination extents, innermost first: (last axis) * C / 4, the axis before it, the one before that
    int ot[3];          // source extents in the same order
    int step[3];        // the low three digits of the loop stride gridDim.x * 256 in the radices `it` ...
    int64_t step3;      // ... and its top digit
};

// EMBED: the destination is the padded tensor (ot <= it; outside the source's extents it is zero).  Else the dense one (ot >= it).
template <bool EMBED>
__global__ __launch_bounds__(kPadBlock) void pad_map_kernel(const float4* __restrict__ src, float4* __restrict__ dst, PadArgs a) {
    int64_t e = (int64_t)blockIdx.x * kPadBlock + threadIdx.x;
    if (e >= a.total) return;
    int d0, d1, d2;
    int64_t d3;
    {
        uint32_t r = (uint32_t)e;      // e < gridDim.x * 256 <= 2^19 here
        d0 = (int)(r % (uint32_t)a.it[0]);
        r /= (uint32_t)a.it[0];
        d1 = (int)(r % (uint32_t)a.it[1]);
        r /= (uint32_t)a.it[1];
        d2 = (int)(r % (uint32_t)a.it[2]);
        d3 = r / (uint32_t)a.it[2];
    }
    const int64_t stride = (int64_t)gridDim.x * kPadBlock;
    for (; e < a.total; e += stride) {
        const int64_t o = ((d3 * a.ot[2] + d2) * a.ot[1] + d1) * (int64_t)a.ot[0] + d0;
        if (EMBED) {
            const bool in = d0 < a.ot[0] && d1 < a.ot[1] && d2 < a.ot[2];
            dst[e] = in ? src[o] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            dst[e] = src[o];
        }
        d0 += a.step[0];
        int c = d0 >= a.it[0];
        d0 -= c ? a.it[0] : 0;
        d1 += a.step[1] + c;
        c = d1 >= a.it[1];
        d1 -= c ? a.it[1] : 0;
        d2 += a.step[2] + c;
        c = d2 >= a.it[2];
        d2 -= c ? a.it[2] : 0;
        d3 += a.step3 + c;
    }
}

static inline bool pad_shape_ok(int nd, const int* sizes, const int* pads, int C) {
    if (nd < 1 || nd > 3 || !sizes || !pads || C < 4 || C % 4 != 0) return false;
    for (int d = 0; d < nd; ++d)
        if (sizes[d] < 1 || pads[d] < 0 || (int64_t)sizes[d] + pads[d] > (1 << 24)) return false;
    return ((int64_t)sizes[nd - 1] + pads[nd - 1]) * (C / 4) < (1LL << 30);      // (a digit plus a stride digit stays an int)
}

static int pad_launch(const float* src, float* dst, long B, int nd, const int* sizes, const int* pads, int C, bool embed, void* stream) {
    if (!src || !dst || B < 1) return FFNO_EINVAL;
    if (!pad_shape_ok(nd, sizes, pads, C)) return FFNO_EUNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) != 0) return FFNO_EINVAL;
    // extents innermost first; the axes a shorter tensor does not have are 1, the batch (and nothing else) goes to the top digit
    int dense[3] = {1, 1, 1}, padded[3] = {1, 1, 1};
    for (int i = 0; i < nd; ++i) {
        dense[i] = sizes[nd - 1 - i];
        padded[i] = sizes[nd - 1 - i] + pads[nd - 1 - i];
    }
    dense[0] *= C / 4;
    padded[0] *= C / 4;
    PadArgs a;
    double elems = (double)B;
    a.total = B;
    for (int i = 0; i < 3; ++i) {
        a.it[i] = embed ? padded[i] : dense[i];
        a.ot[i] = embed ? dense[i] : padded[i];
        a.total *= a.it[i];
        elems *= padded[i];
    }
    if (elems >= (double)(1LL << 40)) return FFNO_EUNSUPPORTED;      // (the padded tensor is the larger: both offsets stay in 64 bits)
    const int64_t blocks = std::min<int64_t>((a.total + kPadBlock - 1) / kPadBlock, kPadMaxBlocks);
    int64_t s = blocks * kPadBlock;
    for (int i = 0; i < 3; ++i) {
        a.step[i] = (int)(s % a.it[i]);
        s /= a.it[i];
    }
    a.step3 = s;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    if (embed)
        FFNO_LAUNCH(pad_map_kernel<true>, dim3((unsigned)blocks), dim3(kPadBlock), 0, (hipStream_t)stream, s4, d4, a);
    else
        FFNO_LAUNCH(pad_map_kernel<false>, dim3((unsigned)blocks), dim3(kPadBlock), 0, (hipStream_t)stream, s4, d4, a);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? FFNO_OK : (int)err;
}

}  // namespace ffno

extern "C" int ffno_pad_supported(int nd, const int* sizes, const int* pads, int C) {
    return ffno::pad_shape_ok(nd, sizes, pads, C) ? 1 : 0;
}

extern "C" int ffno_pad_embed(const float* dense, float* padded, long B, int nd, const int* sizes, const int* pads, int C, void* stream) {
    return ffno::pad_launch(dense, padded, B, nd, sizes, pads, C, true, stream);
}

extern "C" int ffno_pad_crop(const float* padded, float* dense, long B, int nd, const int* sizes, const int* pads, int C, void* stream) {
    return ffno::pad_launch(padded, dense, B, nd, sizes, pads, C, false, stream);
}
