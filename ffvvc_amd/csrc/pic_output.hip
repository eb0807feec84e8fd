// The hand-over of a decoded picture for gfx950 (vvc355_pic_output_pass): crop, repack and change the sample size of the planes where they
// lie — planar or semi-planar (NV12 / P010 family, libavutil/pixdesc.c), as stored, widened to the high bits of 16 (swscale_unscaled.c:237-264)
// or rounded to 8 bit.  A streaming pass: every source byte is read once and every destination byte written once; only the address pattern
// can be done well or badly.
//
// One launch, worked from the DESTINATION's 16-byte grid.  A row of an output plane is cut at every 4 KiB of ADDRESS from the 16-byte line
// its first byte lies in, as pic_digest.hip cuts the rows it reads: a segment is at most 256 sixteen-byte slots, four per lane.  A slot that
// lies whole in the row is one aligned 16-byte store; only the first slot of a row (its head) and the last (its tail) can be partial, and
// those are written sample by sample: nothing outside the rows is written, pitch padding included.  The samples of a whole slot lie
// anywhere in the source (the crop offset is any number of samples, and Cb and Cr need not agree), so a lane fetches them with ONE load of
// exactly their bytes at the alignment of a sample: nothing outside the source rectangle is read, and the hardware splits a load that
// straddles a cache line.  All four loads of a lane are issued before the first store.  Widening, rounding and the interleave of the two
// chroma streams happen in registers (packed 16-bit shifts, v_perm_b32); no LDS, no atomics, vector stores only.
//
// A semi-planar chroma row whose first byte is not a multiple of two samples from its 16-byte line starts its slots with the SECOND
// component of a pair: the even positions of a slot are then the second component from pair x and the odd ones the first from pair x + 1.
// That is wave-uniform (it depends on the row), so the slot is always "two contiguous streams interleaved".
//
// The segments of the picture are dealt round-robin to the waves of the grid, so that the waves in flight work on neighbouring addresses.
#include "common.hpp"
#include "../../include/vvc_mi355.h"
#include <algorithm>

namespace vvc355 {

constexpr int kOutSeg = 4096;              // bytes of destination address per segment: 4 slots of 16 bytes per lane
constexpr int kOutMaxGroups = 1 << 16;     // workgroups at most, 4 waves each: a wave of a larger picture takes several segments

// how a sample changes: 8 -> 8 as stored; 16 -> 16 shifted left by `sh` (0: as stored); 8 -> 16 in the high byte; 16 -> 8 rounded by `sh` bits
enum { OUT_COPY8 = 0, OUT_SHIFT16 = 1, OUT_WIDEN = 2, OUT_NARROW = 3 };

template <typename T, int N> struct Vec { typedef T type __attribute__((ext_vector_type(N))); };
template <int KIND> struct OutKind {
    typedef typename Px<(KIND == OUT_COPY8 || KIND == OUT_WIDEN) ? 8 : 16>::type src_t;
    typedef typename Px<(KIND == OUT_COPY8 || KIND == OUT_NARROW) ? 8 : 16>::type dst_t;
};

// N samples at an address that is aligned to a sample only: one load of exactly their bytes
template <typename T, int N> __device__ __forceinline__ typename Vec<T, N>::type ld_samples(uint64_t addr)
{
    typedef typename Vec<T, N>::type __attribute__((aligned(sizeof(T)))) unaligned_t;
    return *(const VVC355_GLOBAL unaligned_t *)addr;
}

template <int KIND, int N>
__device__ __forceinline__ typename Vec<typename OutKind<KIND>::dst_t, N>::type out_convert(typename Vec<typename OutKind<KIND>::src_t, N>::type s, int sh)
{
    typedef typename Vec<uint16_t, N>::type u16_t;
    if constexpr (KIND == OUT_COPY8) {
        return s;
    } else if constexpr (KIND == OUT_SHIFT16) {
        return s << (u16_t)(uint16_t)sh;                                // 16-bit lanes: what leaves the 16 bits is dropped
    } else if constexpr (KIND == OUT_WIDEN) {
        return __builtin_convertvector(s, u16_t) << (u16_t)(uint16_t)8;
    } else {
        // (S + (1 << (sh - 1))) >> sh without the carry out of 16 bits that S = 0xFFFF would have
        const u16_t r = (s >> (u16_t)(uint16_t)sh) + ((s >> (u16_t)(uint16_t)(sh - 1)) & (u16_t)(uint16_t)1);
        return __builtin_convertvector(__builtin_elementwise_min(r, (u16_t)(uint16_t)255), typename Vec<uint8_t, N>::type);
    }
}

template <int KIND> __device__ __forceinline__ uint32_t out_one(uint32_t s, int sh)
{
    if (KIND == OUT_COPY8)
        return s;
    if (KIND == OUT_SHIFT16)
        return (s << sh) & 0xFFFF;
    if (KIND == OUT_WIDEN)
        return s << 8;
    return min((s + (1u << (sh - 1))) >> sh, 255u);
}

// e0 o0 e1 o1 ...
template <typename T> __device__ __forceinline__ typename Vec<T, 8>::type out_interleave(typename Vec<T, 4>::type e, typename Vec<T, 4>::type o)
{
    return __builtin_shufflevector(e, o, 0, 4, 1, 5, 2, 6, 3, 7);
}
template <typename T> __device__ __forceinline__ typename Vec<T, 16>::type out_interleave(typename Vec<T, 8>::type e, typename Vec<T, 8>::type o)
{
    return __builtin_shufflevector(e, o, 0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15);
}

// segments of one destination row of `rowbytes` bytes, wherever in its 16-byte line the row starts
__host__ __device__ constexpr int out_row_segs(int rowbytes) { return (rowbytes + 15 + kOutSeg - 1) / kOutSeg; }

// One segment by one wave: segment `s` of the destination row at address `drow`, `rowbytes` bytes.  PAIR: the row interleaves the source
// rows srow0 (sample index 2x) and srow1 (2x + 1); otherwise it is the source row srow0.  A segment past the row's end (only a row that
// starts late in its line has one) is empty.
template <int KIND, bool PAIR>
__device__ __forceinline__ void out_segment(uint64_t drow, int rowbytes, int s, uint64_t srow0, uint64_t srow1, int sh, int lane)
{
    typedef typename OutKind<KIND>::src_t src_t;
    typedef typename OutKind<KIND>::dst_t dst_t;
    constexpr int SPX = sizeof(src_t), DPX = sizeof(dst_t), N = 16 / DPX;          // N destination samples per slot
    typedef typename Vec<dst_t, N>::type slot_t;
    const uint64_t line = (drow & ~(uint64_t)15) + (uint64_t)s * kOutSeg;           // slot 0 of the segment
    const int rel = (int)(int64_t)(line - drow);                                    // byte offset of slot 0 in the row (negative in a head)
    const int first = max(-rel, 0);                                                 // byte offsets from `line`: [first, last)
    const int last = min(rowbytes - rel, kOutSeg);
    if (last <= first)
        return;
    // the row's first slot may start with the second component of a pair: wave-uniform
    const bool odd = PAIR && (((rel + 16) / DPX) & 1);
    const uint64_t even_row = odd ? srow1 : srow0, odd_row = odd ? srow0 + SPX : srow1;

    // every load of the segment before any store
    slot_t v[4];
    int cnt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int off = (j * 64 + lane) * 16;
        cnt[j] = min(off + 16, last) - max(off, first);
        if (cnt[j] == 16) {
            const int jd = (rel + off) / DPX;                                       // the slot's first sample in the row; >= 0 here
            if constexpr (PAIR) {
                const uint64_t at = (uint64_t)(jd >> 1) * SPX;
                v[j] = out_interleave<dst_t>(out_convert<KIND, N / 2>(ld_samples<src_t, N / 2>(even_row + at), sh),
                                             out_convert<KIND, N / 2>(ld_samples<src_t, N / 2>(odd_row + at), sh));
            } else {
                v[j] = out_convert<KIND, N>(ld_samples<src_t, N>(srow0 + (uint64_t)jd * SPX), sh);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int off = (j * 64 + lane) * 16;
        if (cnt[j] == 16) {
            // a plain store: __builtin_nontemporal_store here was never faster and 0.5 us slower on an 8K picture's 16-bit modes
            *(VVC355_GLOBAL slot_t *)(line + off) = v[j];
        } else if (cnt[j] > 0) {
            // a head or a tail: its samples one by one
            for (int b = max(off, first); b < min(off + 16, last); b += DPX) {
                const int jd = (rel + b) / DPX;
                const uint64_t from = PAIR ? ((jd & 1) ? srow1 : srow0) + (uint64_t)(jd >> 1) * SPX : srow0 + (uint64_t)jd * SPX;
                gst<dst_t>((void *)(line + b), (dst_t)out_one<KIND>(gld<src_t>((const void *)from), sh));
            }
        }
    }
}

// SEMI: plane 1 interleaves components 1 and 2 (2 and 1 with VVC355_OUT_SWAP_UV) and there is no plane 2
template <int KIND, bool SEMI>
__global__ __launch_bounds__(256) void pic_output_kernel(const vvc355_pic_output_frame *__restrict__ fp, uint32_t n_segs, int sh)
{
    constexpr int DPX = sizeof(typename OutKind<KIND>::dst_t);
    const vvc355_pic_output_frame f = load_uniform(fp);
    const int lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int n_planes = SEMI ? 2 : f.n_comp;
    // the pair's first and second component (selects, not indexed: the frame lives in scalar registers)
    const bool swap = f.flags & VVC355_OUT_SWAP_UV;
    const uint64_t src0 = swap ? f.src[2] : f.src[1], src1 = swap ? f.src[1] : f.src[2];
    const int stride0 = swap ? f.src_stride[2] : f.src_stride[1], stride1 = swap ? f.src_stride[1] : f.src_stride[2];
    for (uint32_t i = wave; i < n_segs; i += n_waves) {
        uint32_t base = 0;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            if (p >= n_planes)
                break;
            const bool pair = SEMI && p == 1;
            const int rowbytes = f.width[p] * DPX * (pair ? 2 : 1), per_row = out_row_segs(rowbytes);
            const uint32_t n_p = (uint32_t)f.height[p] * per_row;
            if (i - base < n_p) {
                const int y = (int)((i - base) / per_row), s = (int)((i - base) - (uint32_t)y * per_row);
                const uint64_t drow = f.dst[p] + (uint64_t)((int64_t)y * f.dst_stride[p]);
                if (pair)
                    out_segment<KIND, true>(drow, rowbytes, s, src0 + (uint64_t)((int64_t)y * stride0), src1 + (uint64_t)((int64_t)y * stride1), sh, lane);
                else
                    out_segment<KIND, false>(drow, rowbytes, s, f.src[p] + (uint64_t)((int64_t)y * f.src_stride[p]), 0, sh, lane);
                break;
            }
            base += n_p;
        }
    }
}

// [a, a + an) and [b, b + bn) share a byte
static bool out_spans_meet(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return a < b + bn && b < a + an; }

// the frame as the header states it, every refusal before any HIP call; *n_segs = the picture's segments
static int pic_output_check(const vvc355_pic_output_frame *f, int bd, uint32_t *n_segs)
{
    if (!f || (f->n_comp != 1 && f->n_comp != 3))
        return VVC355_PIC_OUTPUT_E_FRAME;
    if (bd != 8 && bd != 10 && bd != 12)
        return VVC355_PIC_OUTPUT_E_BD;
    const bool semi = f->layout == VVC355_OUT_SEMI;
    if ((f->layout != VVC355_OUT_PLANAR && !semi) || (f->out_bits != bd && f->out_bits != 16 && f->out_bits != 8))
        return VVC355_PIC_OUTPUT_E_FORMAT;
    if ((f->flags & ~VVC355_OUT_SWAP_UV) || (f->flags && !semi) || f->pad_[0] || f->pad_[1] || f->pad_[2] || f->pad_[3])
        return VVC355_PIC_OUTPUT_E_FORMAT;
    if (semi && (f->n_comp != 3 || f->width[1] != f->width[2] || f->height[1] != f->height[2] || f->dst[2]))
        return VVC355_PIC_OUTPUT_E_FORMAT;
    for (int c = 0; c < f->n_comp; c++)
        if (f->width[c] <= 0 || f->height[c] <= 0 || f->width[c] >= (1 << 16) || f->height[c] >= (1 << 16))
            return VVC355_PIC_OUTPUT_E_SIZE;
    const int spx = bd > 8 ? 2 : 1, dpx = f->out_bits > 8 ? 2 : 1;
    const int n_planes = semi ? 2 : f->n_comp;
    int drow[3] = { 0, 0, 0 };                                                      // bytes of a row of output plane p
    for (int p = 0; p < n_planes; p++)
        drow[p] = f->width[p] * dpx * (semi && p == 1 ? 2 : 1);                     // <= 65535 * 4
    auto bad_stride = [](int32_t stride, int row, int px, int height) {
        return stride < row || stride % px || stride >= (1 << 23) || (int64_t)stride * height >= ((int64_t)1 << 31);
    };
    for (int c = 0; c < f->n_comp; c++)
        if (bad_stride(f->src_stride[c], f->width[c] * spx, spx, f->height[c]))
            return VVC355_PIC_OUTPUT_E_STRIDE;
    uint64_t n = 0;
    for (int p = 0; p < n_planes; p++) {
        if (bad_stride(f->dst_stride[p], drow[p], dpx, f->height[p]))
            return VVC355_PIC_OUTPUT_E_STRIDE;
        n += (uint64_t)f->height[p] * out_row_segs(drow[p]);                        // < 3 * 2^16 * 65
    }
    for (int c = 0; c < f->n_comp; c++)
        if (!f->src[c] || f->src[c] % spx)
            return VVC355_PIC_OUTPUT_E_PLANES;
    for (int p = 0; p < n_planes; p++)
        if (!f->dst[p] || f->dst[p] % dpx)
            return VVC355_PIC_OUTPUT_E_PLANES;
    for (int p = 0; p < n_planes; p++)
        for (int c = 0; c < f->n_comp; c++)
            if (out_spans_meet(f->dst[p], (uint64_t)f->dst_stride[p] * (f->height[p] - 1) + drow[p],
                               f->src[c], (uint64_t)f->src_stride[c] * (f->height[c] - 1) + (uint64_t)f->width[c] * spx))
                return VVC355_PIC_OUTPUT_E_OVERLAP;
    *n_segs = (uint32_t)n;
    return 0;
}

} // namespace vvc355

using namespace vvc355;

extern "C" {

int vvc355_pic_output_pass(void *stream, int bd, const vvc355_pic_output_frame *frame_dev, const vvc355_pic_output_frame *frame_host)
{
    uint32_t n_segs = 0;
    const int err = frame_dev ? pic_output_check(frame_host, bd, &n_segs) : VVC355_PIC_OUTPUT_E_FRAME;
    if (err)
        return err;
    const int groups = (int)std::min((n_segs + 3) / 4, (uint32_t)kOutMaxGroups);
    const int out_bits = frame_host->out_bits;
    const int kind = bd == 8 ? (out_bits == 8 ? OUT_COPY8 : OUT_WIDEN) : (out_bits == 8 ? OUT_NARROW : OUT_SHIFT16);
    const int sh = kind == OUT_NARROW ? bd - 8 : kind == OUT_SHIFT16 ? out_bits - bd : 0;
#define OUT_LAUNCH(KIND, SEMI) \
    hipLaunchKernelGGL((pic_output_kernel<KIND, SEMI>), dim3(groups), dim3(256), 0, (hipStream_t)stream, frame_dev, n_segs, sh)
#define OUT_CASE(KIND) \
    case KIND: if (frame_host->layout == VVC355_OUT_SEMI) OUT_LAUNCH(KIND, true); else OUT_LAUNCH(KIND, false); break
    switch (kind) { OUT_CASE(OUT_COPY8); OUT_CASE(OUT_SHIFT16); OUT_CASE(OUT_WIDEN); OUT_CASE(OUT_NARROW); }
#undef OUT_CASE
#undef OUT_LAUNCH
    HIP_CHECK(hipGetLastError());
    return 0;
}

} // extern "C"
