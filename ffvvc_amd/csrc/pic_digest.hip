// The checksums of a decoded picture for gfx950 (vvc355_pic_digest_pass): Adler-32 with start value 0 (libavformat/framecrcenc.c:53), and the
// picture_checksum and picture_crc of the decoded picture hash SEI (Rec. ITU-T H.274 §8.8.2), all from one read of the planes.
//
// All three split into pieces that combine exactly, and the same element describes a piece at every level (lane, segment, wave, picture):
//   Adler   (A, B, len):   A = A1 + A2,  B = B1 + B2 + (len2 mod 65521) * A1,  all modulo 65521 (start value 0, so no constant terms);
//   CRC     (crc, xp):     the register run from 0 and xp = x^(8 len) mod P;  crc = crc1 * xp2 ^ crc2,  xp = xp1 * xp2  over GF(2)[x] / P,
//                          P = x^16 + x^12 + x^5 + 1.  The initial value is folded in once per plane: 0x1D0F * xp ^ crc;
//   checksum               a 32-bit wrapping sum; the mask of a sample depends on its coordinates only.
// MD5, the SEI's third form, chains 64-byte blocks serially per component and is left out.
//
// Two launches.  pic_digest_partial_kernel: a row of a component is cut at every 4 KiB of ADDRESS from the 16-byte line its first byte
// lies in, so a segment is at most 256 sixteen-byte slots, one aligned 16-byte load per lane and pass; only the first slot of a row (its
// head) and the last (its tail) can be partial, and those are read byte by byte: nothing outside the rectangle is read.  The segments of
// the picture, in the order of the bytes, are dealt in contiguous shares to the waves of a bounded grid; a wave walks its share, reduces
// a segment across its lanes with plain sums and xors (a lane weights its slot by the bytes that follow it in the segment, which is what
// makes the reduction order-free), appends the segment to its running element; the four waves of a workgroup hold consecutive shares and store one element per component.  No workgroup waits
// for another.  pic_digest_combine_kernel, one workgroup: the elements of a component in order, a few per lane and then a tree, the components side by side, then the
// planes in order for the picture's Adler-32, and the result written whole.
#include "common.hpp"
#include "../../include/vvc_mi355.h"
#include <algorithm>

namespace vvc355 {

constexpr int kDigestSeg = 4096;           // bytes of address per segment: 4 slots of 16 bytes per lane
constexpr int kDigestMaxGroups = 2048;     // workgroups of the partials kernel at most: 4 waves each, 8 per CU
constexpr int kDigestSegsPerGroup = 8;     // a smaller picture gets fewer workgroups: two segments per wave where there are that many
constexpr int kDigestPartDwords = 5;       // a, b, len, crc | xp << 16, checksum
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kCrcInit = 0x1D0F;      // the SEI's 0xFFFF register with its 16 appended zero bits, as a direct-form initial value

// a * b in GF(2)[x] / P, both below 2^16
__host__ __device__ constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x8000) ? 0x11021u : 0u);
        r ^= ((b >> i) & 1) ? a : 0u;
    }
    return r;
}

struct DigestTables {
    uint16_t byte_at[16][256];   // the register (from 0) of a 16-byte slot that holds value b at position p and zeros elsewhere
    uint16_t xp_slot[257];       // x^(8 * 16 * k) mod P
    uint16_t xp_byte[16];        // x^(8 * r) mod P
};

constexpr DigestTables make_digest_tables()
{
    DigestTables t = {};
    for (int b = 0; b < 256; b++) {
        uint32_t r = (uint32_t)b << 8;
        for (int i = 0; i < 8; i++)
            r = ((r << 1) ^ ((r & 0x8000) ? 0x11021u : 0u)) & 0xFFFF;
        t.byte_at[15][b] = (uint16_t)r;
    }
    for (int p = 14; p >= 0; p--)
        for (int b = 0; b < 256; b++) {
            const uint32_t r = t.byte_at[p + 1][b];
            t.byte_at[p][b] = (uint16_t)(((r << 8) & 0xFFFF) ^ t.byte_at[15][r >> 8]);
        }
    t.xp_byte[0] = 1;
    for (int r = 1; r < 16; r++)
        t.xp_byte[r] = (uint16_t)crc_mulmod(t.xp_byte[r - 1], 0x0100);
    const uint32_t x128 = crc_mulmod(t.xp_byte[15], 0x0100);
    t.xp_slot[0] = 1;
    for (int k = 1; k < 257; k++)
        t.xp_slot[k] = (uint16_t)crc_mulmod(t.xp_slot[k - 1], x128);
    return t;
}

__device__ const DigestTables kDigestTables = make_digest_tables();

// the element of a run of bytes; the empty run is { 0, 0, 0, 0, 1, 0 }
struct DigestPart {
    uint32_t a, b, len, crc, xp, sum;
};

// `l` followed by `r`
template <int WHAT>
__device__ __forceinline__ DigestPart digest_join(const DigestPart &l, const DigestPart &r)
{
    DigestPart o = { 0, 0, l.len + r.len, 0, 1, 0 };
    if (WHAT & VVC355_DIGEST_ADLER32) {
        o.a = (l.a + r.a) % kAdlerMod;
        o.b = (l.b + r.b + (r.len % kAdlerMod) * l.a % kAdlerMod) % kAdlerMod;     // (len mod 65521) * A < 2^32
    }
    if (WHAT & VVC355_DIGEST_CRC) {
        o.crc = crc_mulmod(l.crc, r.xp) ^ r.crc;
        o.xp = crc_mulmod(l.xp, r.xp);
    }
    if (WHAT & VVC355_DIGEST_CHECKSUM)
        o.sum = l.sum + r.sum;
    return o;
}

__device__ __forceinline__ void digest_store(uint32_t *p, const DigestPart &e)
{
    gst<uint32_t>(p + 0, e.a);
    gst<uint32_t>(p + 1, e.b);
    gst<uint32_t>(p + 2, e.len);
    gst<uint32_t>(p + 3, e.crc | e.xp << 16);
    gst<uint32_t>(p + 4, e.sum);
}

__device__ __forceinline__ DigestPart digest_load(const uint32_t *p)
{
    const uint32_t cx = gld<uint32_t>(p + 3);
    return DigestPart{ gld<uint32_t>(p + 0), gld<uint32_t>(p + 1), gld<uint32_t>(p + 2), cx & 0xFFFF, cx >> 16, gld<uint32_t>(p + 4) };
}

__device__ __forceinline__ uint32_t wave_add(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
        v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
        v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// segments of one row of `rowbytes` bytes, wherever in its 16-byte line the row starts
__host__ __device__ constexpr int digest_row_segs(int rowbytes) { return (rowbytes + 15 + kDigestSeg - 1) / kDigestSeg; }

// One segment by one wave: segment `s` of the row at address `row`.  Returns its element in every lane (the empty one for a segment past
// the row's end, which only a row that starts late in its line has).  y is the row's number in the component, for the checksum's mask.
template <int PXB, int WHAT>
__device__ __forceinline__ DigestPart digest_segment(uint64_t row, int rowbytes, int s, int y, int lane, const uint16_t *byte_at, const uint16_t *xp_slot)
{
    DigestPart e = { 0, 0, 0, 0, 1, 0 };
    const uint64_t line = (row & ~(uint64_t)15) + (uint64_t)s * kDigestSeg;       // slot 0 of the segment
    const int first = max((int)(row - line), 0);                                    // byte offsets from `line`: [first, last)
    const int last = (int)min((int64_t)(row + rowbytes - line), (int64_t)kDigestSeg);
    if (last <= first)
        return e;
    const int n_whole = last >> 4, tail = last & 15;                                // slots in front of the tail slot; bytes of the tail slot
    const int x_line = (int)(int64_t)(line - row);                                  // byte offset of slot 0 in the row (negative in a head)
    const uint32_t ymask = (y & 0xFF) ^ (y >> 8);
    uint32_t a_sum = 0, b_sum = 0, crc_pack = 0, sum = 0;

    // every load of the segment before any use
    uint4 w[4];
    int cnt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int off = (j * 64 + lane) * 16;
        const int lo = max(off, first), hi = min(off + 16, last);
        cnt[j] = hi - lo;
        w[j] = make_uint4(0, 0, 0, 0);
        if (cnt[j] == 16) {
            w[j] = gld<uint4>((const void *)(line + off));
        } else if (cnt[j] > 0) {
            // a head or a tail: its bytes one by one, moved to the END of the slot (zeros in front change neither Adler from 0, nor a
            // CRC register that starts at 0, and carry weight 0 in the checksum)
            uint64_t v_lo = 0, v_hi = 0;
            for (int i = 0; i < cnt[j]; i++) {
                const uint64_t b = gld<uint8_t>((const void *)(line + lo + i));
                v_lo = (v_lo >> 8) | (v_hi << 56);
                v_hi = (v_hi >> 8) | (b << 56);
            }
            w[j] = make_uint4((uint32_t)v_lo, (uint32_t)(v_lo >> 32), (uint32_t)v_hi, (uint32_t)(v_hi >> 32));
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int n = cnt[j];
        if (n <= 0)
            continue;
        const int off = (j * 64 + lane) * 16;
        const int hi = min(off + 16, last);
        const uint32_t d[4] = { w[j].x, w[j].y, w[j].z, w[j].w };
        if (WHAT & VVC355_DIGEST_ADLER32) {
            // over the slot: s1 = sum of b, s2 = sum of (16 - position) * b; then B of the segment takes s2 + (bytes after the slot) * s1
            uint32_t s1 = 0, s2 = 0;
            s1 = dot4(d[0], 0x01010101u, s1); s2 = dot4(d[0], 0x0D0E0F10u, s2);
            s1 = dot4(d[1], 0x01010101u, s1); s2 = dot4(d[1], 0x090A0B0Cu, s2);
            s1 = dot4(d[2], 0x01010101u, s1); s2 = dot4(d[2], 0x05060708u, s2);
            s1 = dot4(d[3], 0x01010101u, s1); s2 = dot4(d[3], 0x01020304u, s2);
            a_sum += s1;                                                            // <= 4 * 16 * 255
            b_sum += s2 + (uint32_t)(last - hi) * s1;                               // <= 4 * (34 680 + 4 096 * 4 080) < 2^27
        }
        if (WHAT & VVC355_DIGEST_CRC) {
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    c ^= byte_at[(k * 4 + i) * 256 + ((d[k] >> (8 * i)) & 0xFF)];
            const int slot = j * 64 + lane;
            if (slot < n_whole)
                crc_pack ^= crc_mulmod(c, xp_slot[n_whole - 1 - slot]);            // whole slots follow it, then the tail
            else
                crc_pack ^= c << 16;                                                // the tail slot itself
        }
        if (WHAT & VVC355_DIGEST_CHECKSUM) {
            const int pad = 16 - n;
            // sample coordinate of position 0 of the slot as it stands in w (the bytes of a partial slot were moved to its end)
            const int x0 = (x_line + max(off, first) - pad) / PXB;                  // exact: everything is a multiple of PXB
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t m;
                if (PXB == 1) {
                    m = 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int x = x0 + 4 * k + i;
                        m |= ((uint32_t)(x ^ (x >> 8) ^ ymask) & 0xFF) << (8 * i);
                    }
                } else {
                    const int xa = x0 + 2 * k, xb = xa + 1;
                    m = (((uint32_t)(xa ^ (xa >> 8) ^ ymask) & 0xFF) | ((uint32_t)(xb ^ (xb >> 8) ^ ymask) & 0xFF) << 16) * 0x0101u;
                }
                const int p = min(max(pad - 4 * k, 0), 4);                          // positions of this dword that hold no byte
                const uint32_t valid = p >= 4 ? 0u : 0x01010101u << (8 * p);
                sum = dot4(d[k] ^ m, valid, sum);
            }
        }
    }
    e.len = (uint32_t)(last - first);
    if (WHAT & VVC355_DIGEST_ADLER32) {
        e.a = wave_add(a_sum) % kAdlerMod;                                          // <= 4 096 * 255
        e.b = wave_add(b_sum % kAdlerMod) % kAdlerMod;
    }
    if (WHAT & VVC355_DIGEST_CRC) {
        const uint32_t p = wave_xor(crc_pack);
        const uint32_t body = p & 0xFFFF;
        e.crc = (tail ? crc_mulmod(body, gld<uint16_t>(&kDigestTables.xp_byte[tail])) : body) ^ (p >> 16);
        e.xp = crc_mulmod(xp_slot[e.len >> 4], gld<uint16_t>(&kDigestTables.xp_byte[e.len & 15]));
    }
    if (WHAT & VVC355_DIGEST_CHECKSUM)
        e.sum = wave_add(sum);
    return e;
}

// work: n_comp arrays of gridDim.x elements, one per workgroup
template <int PXB, int WHAT>
__global__ __launch_bounds__(256) void pic_digest_partial_kernel(const vvc355_pic_digest_frame *__restrict__ fp, uint32_t n_segs)
{
    __shared__ uint16_t byte_at[16 * 256];
    __shared__ uint16_t xp_slot[257 + 7];
    __shared__ DigestPart wave_run[4];
    if (WHAT & VVC355_DIGEST_CRC) {
        static_assert(sizeof(kDigestTables.byte_at) == 256 * 32 && sizeof(kDigestTables.byte_at) % 16 == 0, "staged with 16-byte loads");
        for (int i = threadIdx.x; i < (int)sizeof(kDigestTables.byte_at) / 16; i += 256)
            ((uint4 *)byte_at)[i] = gld<uint4>((const uint8_t *)kDigestTables.byte_at + i * 16);
        for (int i = threadIdx.x; i < 257; i += 256)
            xp_slot[i] = gld<uint16_t>(&kDigestTables.xp_slot[i]);
        __syncthreads();
    }
    const vvc355_pic_digest_frame f = load_uniform(fp);
    const int lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    // this wave's share of the picture's segments, in the order of the bytes
    const uint32_t share_lo = (uint32_t)((uint64_t)wave * n_segs / n_waves), share_hi = (uint32_t)((uint64_t)(wave + 1) * n_segs / n_waves);
    uint32_t *work = (uint32_t *)f.work;
    uint32_t base = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c >= f.n_comp)
            break;
        const int rowbytes = f.width[c] * PXB, per_row = digest_row_segs(rowbytes);
        const uint32_t n_c = (uint32_t)f.height[c] * per_row;
        const uint32_t lo = max(share_lo, base), hi = min(share_hi, base + n_c);
        DigestPart run = { 0, 0, 0, 0, 1, 0 };
        if (lo < hi) {
            int y = (int)((lo - base) / per_row), s = (int)((lo - base) - (uint32_t)y * per_row);
            for (uint32_t i = lo; i < hi; i++) {
                const DigestPart e = digest_segment<PXB, WHAT>(f.plane[c] + (uint64_t)((int64_t)y * f.stride[c]), rowbytes, s, y, lane, byte_at, xp_slot);
                run = digest_join<WHAT>(run, e);
                if (++s == per_row) {
                    s = 0;
                    y++;
                }
            }
        }
        // the four waves' shares follow one another: one element per workgroup and component
        if (lane == 0)
            wave_run[threadIdx.x >> 6] = run;
        __syncthreads();
        if (threadIdx.x == 0) {
            DigestPart all = wave_run[0];
            for (int v = 1; v < 4; v++)
                all = digest_join<WHAT>(all, wave_run[v]);
            digest_store(work + ((size_t)c * gridDim.x + blockIdx.x) * kDigestPartDwords, all);
        }
        __syncthreads();
        base += n_c;
    }
}

// One workgroup, 256 lanes per component: the n_parts <= kDigestMaxGroups elements of a component in order — a lane loads its few (every
// load issued before the first join), joins them, then a tree over the 256 — then lane 0 writes the result.  ALL: the digests the elements
// may carry (the CRC's joins are the expensive ones, so a call without it gets a kernel without them).
template <int ALL>
__global__ __launch_bounds__(768) void pic_digest_combine_kernel(const vvc355_pic_digest_frame *__restrict__ fp, uint32_t n_parts)
{
    constexpr int PER = kDigestMaxGroups / 256;
    __shared__ DigestPart tree[3][256];
    const vvc355_pic_digest_frame f = load_uniform(fp);
    const uint32_t *work = (const uint32_t *)f.work;
    const int comp = threadIdx.x >> 8, t = threadIdx.x & 255;         // blockDim.x = 256 * n_comp
    {
        const uint32_t lo = (uint32_t)t * n_parts / 256, hi = (uint32_t)(t + 1) * n_parts / 256;      // at most PER of them
        DigestPart e[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            // a load that is not this lane's goes to an element that exists and is dropped: no load waits for a branch
            e[k] = digest_load(work + ((size_t)comp * n_parts + min(lo + k, n_parts - 1)) * kDigestPartDwords);
            if (lo + k >= hi)
                e[k] = DigestPart{ 0, 0, 0, 0, 1, 0 };
        }
        DigestPart run = e[0];
#pragma unroll
        for (int k = 1; k < PER; k++)
            run = digest_join<ALL>(run, e[k]);
        tree[comp][t] = run;
    }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        if ((t & (2 * d - 1)) == 0)
            tree[comp][t] = digest_join<ALL>(tree[comp][t], tree[comp][t + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        uint32_t *out = (uint32_t *)f.result;
        const bool adler = f.what & VVC355_DIGEST_ADLER32, sum = f.what & VVC355_DIGEST_CHECKSUM, crc = f.what & VVC355_DIGEST_CRC;
        DigestPart all = { 0, 0, 0, 0, 1, 0 };
        uint32_t plane_adler[3] = { 0, 0, 0 }, checksum[3] = { 0, 0, 0 }, crcs[3] = { 0, 0, 0 };
        for (int c = 0; c < f.n_comp; c++) {
            const DigestPart p = tree[c][0];
            all = digest_join<VVC355_DIGEST_ADLER32>(all, p);
            plane_adler[c] = adler ? p.b << 16 | p.a : 0;
            checksum[c] = sum ? p.sum : 0;
            crcs[c] = crc ? crc_mulmod(kCrcInit, p.xp) ^ p.crc : 0;
        }
        gst<uint32_t>(out + 0, adler ? all.b << 16 | all.a : 0);
        for (int c = 0; c < 3; c++) {
            gst<uint32_t>(out + 1 + c, plane_adler[c]);
            gst<uint32_t>(out + 4 + c, checksum[c]);
        }
        gst<uint32_t>(out + 7, crcs[0] | crcs[1] << 16);
        gst<uint32_t>(out + 8, crcs[2] | (uint32_t)f.n_comp << 16);
    }
}

// the frame as the header states it, every refusal before any HIP call; *n_segs = the picture's segments
static int pic_digest_check(const vvc355_pic_digest_frame *f, int bd, uint32_t *n_segs)
{
    if (!f || (f->n_comp != 1 && f->n_comp != 3))
        return VVC355_PIC_DIGEST_E_FRAME;
    if (bd != 8 && bd != 10 && bd != 12)
        return VVC355_PIC_DIGEST_E_BD;
    if (!f->what || (f->what & ~7) || f->pad_[0] || f->pad_[1])
        return VVC355_PIC_DIGEST_E_WHAT;
    const int px = bd > 8 ? 2 : 1;
    for (int c = 0; c < f->n_comp; c++)
        if (f->width[c] <= 0 || f->height[c] <= 0 || f->width[c] >= (1 << 16) || f->height[c] >= (1 << 16))
            return VVC355_PIC_DIGEST_E_SIZE;
    uint64_t n = 0;
    for (int c = 0; c < f->n_comp; c++) {
        if (f->stride[c] < f->width[c] * px || f->stride[c] % px || f->stride[c] >= (1 << 23) || (int64_t)f->stride[c] * f->height[c] >= ((int64_t)1 << 31))
            return VVC355_PIC_DIGEST_E_STRIDE;
        n += (uint64_t)f->height[c] * digest_row_segs(f->width[c] * px);            // < 3 * 2^16 * 33
    }
    for (int c = 0; c < f->n_comp; c++)
        if (!f->plane[c] || f->plane[c] % px)
            return VVC355_PIC_DIGEST_E_TABLES;
    if (!f->result || !f->work || f->result % 4 || f->work % 4)
        return VVC355_PIC_DIGEST_E_TABLES;
    *n_segs = (uint32_t)n;
    return 0;
}

static int pic_digest_groups(uint32_t n_segs)
{
    return (int)std::min((n_segs + kDigestSegsPerGroup - 1) / kDigestSegsPerGroup, (uint32_t)kDigestMaxGroups);
}

} // namespace vvc355

using namespace vvc355;

extern "C" {

size_t vvc355_pic_digest_work_bytes(const vvc355_pic_digest_frame *frame_host, int bd)
{
    uint32_t n_segs = 0;
    if (pic_digest_check(frame_host, bd, &n_segs))
        return 0;
    return (size_t)frame_host->n_comp * pic_digest_groups(n_segs) * kDigestPartDwords * sizeof(uint32_t);
}

int vvc355_pic_digest_pass(void *stream, int bd, const vvc355_pic_digest_frame *frame_dev, const vvc355_pic_digest_frame *frame_host)
{
    uint32_t n_segs = 0;
    const int err = frame_dev ? pic_digest_check(frame_host, bd, &n_segs) : VVC355_PIC_DIGEST_E_FRAME;
    if (err)
        return err;
    const int groups = pic_digest_groups(n_segs);
#define DIGEST_LAUNCH(PXB, WHAT) \
    case WHAT: hipLaunchKernelGGL((pic_digest_partial_kernel<PXB, WHAT>), dim3(groups), dim3(256), 0, (hipStream_t)stream, frame_dev, n_segs); break
#define DIGEST_DISPATCH(PXB) \
    switch (frame_host->what) { DIGEST_LAUNCH(PXB, 1); DIGEST_LAUNCH(PXB, 2); DIGEST_LAUNCH(PXB, 3); DIGEST_LAUNCH(PXB, 4); \
                                DIGEST_LAUNCH(PXB, 5); DIGEST_LAUNCH(PXB, 6); DIGEST_LAUNCH(PXB, 7); }
    if (bd > 8)
        DIGEST_DISPATCH(2)
    else
        DIGEST_DISPATCH(1)
#undef DIGEST_DISPATCH
#undef DIGEST_LAUNCH
    HIP_CHECK(hipGetLastError());
    if (frame_host->what & VVC355_DIGEST_CRC)
        hipLaunchKernelGGL((pic_digest_combine_kernel<7>), dim3(1), dim3(256 * frame_host->n_comp), 0, (hipStream_t)stream, frame_dev, (uint32_t)groups);
    else
        hipLaunchKernelGGL((pic_digest_combine_kernel<3>), dim3(1), dim3(256 * frame_host->n_comp), 0, (hipStream_t)stream, frame_dev, (uint32_t)groups);
    HIP_CHECK(hipGetLastError());
    return 0;
}

} // extern "C"
