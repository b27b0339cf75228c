// icx_kernels.hip — CDNA4 (gfx950) kernels for the JPEG target-size path.
//
// Kernel map (reference rows from SURVEY.md §8a; arithmetic restates IJG 6b
// as reached through the JDK writer, see oracle/icx_oracle.c for the CPU
// statement of the same algorithm):
//   k_fdct_color / k_fdct_gray  A7+A8+A9: rgb_ycc_convert, edge expansion,
//                               h2v2_downsample, jpeg_fdct_islow (raw, x8)
//   k_huff                      A9 quantise + A10 Huffman: per-chunk packed
//                               bitstream, one thread per 8x8 block
//   k_scan                      exclusive scan of chunk bit counts; 0xFF bytes
//                               per chunk from the huff kernel's alignment bins
//                               (exact stuffed size without writing it), then
//                               the A3 binary-search step (decide_trial)
//   k_ffscan + k_stuff          final file: header, stuffed bytes, EOI
//   k_resize                    A12 Java2D bilinear (TransformHelper)
// No MFMA: integer, byte-oriented work bound by HBM.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/icx.h"
#include "icx_internal.h"
#include "icx_kernels.h"

namespace icx {

__constant__ uint8_t c_nat_to_zz[64];
__constant__ uint8_t c_zz_to_nat[64];
__constant__ uint32_t c_dc[2][16];    // (code << 8) | length, by category
__constant__ uint32_t c_ac[2][256];   // (code << 8) | length, by run/size symbol
// k_huff's AC table, pre-shifted per (run, size) slot: (code << size, len + size)
// at [run * 11 + size]; built once by upload_constants.
__constant__ uint2 c_acx[2][16 * 11];
__constant__ uint8_t c_hdr[4][HDR_COLOR];  // [grouped * 2 + colour]: grey / colour templates, per table layout

// ------------------------------------------------------------------ helpers
// Pointers read from descriptors are generic; casting them to the global
// address space makes hipcc emit global_load/store instead of flat_* (which
// need a private segment and are waited for on both vmcnt and lgkmcnt).
#define GAS __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ GAS T* gp(T* p) { return (GAS T*)p; }
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 ld16(const void* p)
{
    const u32x4_t v = *(const GAS u32x4_t*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int2 ld8(const void* p)
{
    const i32x2_t v = *(const GAS i32x2_t*)p;
    return make_int2(v.x, v.y);
}
__device__ __forceinline__ void st8(void* p, int2 v)
{
    i32x2_t w;
    w.x = v.x;
    w.y = v.y;
    *(GAS i32x2_t*)p = w;
}
// Launch slot of work item `item` (prefix = exclusive item counts per slot,
// prefix[m] = total).  A proportional guess first - exact when the slots hold
// equally many items, as for a batch of same-sized frames: two dependent loads
// instead of log2(m) - then a binary search of what the guess left open.
// Inclusive prefix sum over the 64 lanes of a wave with DPP moves (row
// shifts within 16-lane rows, then row broadcasts 15 and 31): a few cycles per
// step instead of an LDS-crossbar round trip per __shfl_up.  Every lane must
// be active.
__device__ __forceinline__ int wave_incl_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

__device__ __forceinline__ int find_slot(const int64_t* prefix, int m, int64_t item)
{
    int lo = 0, hi = m;  // prefix[lo] <= item < prefix[hi]
#if !ICX_PLAIN_SLOT_SEARCH
    const int g = min(max((int)(((float)item + 0.5f) * ((float)m / (float)prefix[m])), 0), m - 1);
    if (prefix[g] <= item) {
        lo = g;
        if (item < prefix[g + 1]) return g;
    } else {
        hi = g;
    }
#endif
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

#define CONST_BITS 13
#define PASS1_BITS 2
#define DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

// Two int16 lanes (lo, hi) of one dword, and lo * c0 + hi * c1 + acc in one
// VOP3P v_dot2_i32_i16 (exact: products and sums stay far inside int32).  The
// builtin compiles to the two-address v_dot2c form, which needs a v_mov of
// the accumulator in front of every chain; the three-address form reads the
// coefficient pair from an SGPR and the accumulator from any VGPR.
__device__ __forceinline__ uint32_t pack16(int lo, int hi)
{
    return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u);
}
template <int C0, int C1>
__device__ __forceinline__ int dot2(uint32_t p, int acc)
{
    static_assert(C0 >= -32768 && C0 < 32768 && C1 >= -32768 && C1 < 32768, "int16 weights");
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(p), "s"(((uint32_t)C0 & 0xFFFFu) | ((uint32_t)C1 << 16)), "v"(acc));
    return d;
}

// One 1-D pass of jpeg_fdct_islow (jfdctint.c, IJG 6b).  pass 0 = rows
// (outputs scaled up by PASS1_BITS), pass 1 = columns.
// The rotations are IJG's products expanded per input: e.g. the odd part's
// d7 = t4*2446 + z1*-7373 + z3*-16069 + z5 (z1 = t4+t7, z3 = t4+t6, z5 =
// (t4+t5+t6+t7)*9633) is t4*-11363 + t5*9633 + t6*-6436 + t7*2260 - the same
// integer, so the same DESCALE - i.e. two dot2 ops over (t4, t5), (t6, t7)
// with the rounding constant as the accumulator.  Every t* fits int16 (rows:
// |t| <= 510 from 8-bit samples; columns: row outputs lie in [-4096, 4080],
// so |t| <= 16352), checked at the extreme inputs (tests/test_ycc_identity.py).
// 34 instead of ~48 VALU per pass.
// HI (columns only): every output is left in the high 16 bits of its int32
// (low bits undefined) for a ds_write_b16_d16_hi store - no shift: doubled
// weights (still int16: the largest is 2 * 11363 = 22726) and rounding constant give
// 2x + 2^15, whose bits 16.. are DESCALE(x, 15); d0 / d4 are shifted left
// instead of right.
template <int PASS, bool HI = false>
__device__ __forceinline__ void fdct8(int32_t& d0, int32_t& d1, int32_t& d2, int32_t& d3,
                                      int32_t& d4, int32_t& d5, int32_t& d6, int32_t& d7)
{
    static_assert(!HI || PASS == 1, "high-half outputs for the column pass");
    int32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
    int32_t t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SH = PASS == 0 ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    constexpr int K = HI ? 2 : 1;          // weight scale
    constexpr int OS = HI ? 0 : SH;        // output shift
    constexpr int R = 1 << (SH - 1 + (HI ? 1 : 0));
    if (PASS == 0) {
        d0 = (t10 + t11) << PASS1_BITS;
        d4 = (t10 - t11) << PASS1_BITS;
    } else if (HI) {
        d0 = (t10 + t11 + (1 << (PASS1_BITS - 1))) << (16 - PASS1_BITS);
        d4 = (t10 - t11 + (1 << (PASS1_BITS - 1))) << (16 - PASS1_BITS);
    } else {
        d0 = DESCALE(t10 + t11, PASS1_BITS);
        d4 = DESCALE(t10 - t11, PASS1_BITS);
    }
    int r = R;  // the rounding constant, once in a VGPR for all six chains
    asm("" : "+v"(r));
    // even: z1 = (t12 + t13) * FIX_0_541196100, + t13 * FIX_0_765366865, - t12 * FIX_1_847759065
    const uint32_t e = pack16(t12, t13);
    d2 = dot2<K * 4433, K * 10703>(e, r) >> OS;
    d6 = dot2<K * -10704, K * 4433>(e, r) >> OS;
    // odd: FIX_0_298631336 2446, FIX_2_053119869 16819, FIX_3_072711026 25172,
    // FIX_1_501321110 12299, FIX_0_899976223 7373, FIX_2_562915447 20995,
    // FIX_1_961570560 16069, FIX_0_390180644 3196, FIX_1_175875602 9633
    const uint32_t a = pack16(t4, t5), b = pack16(t6, t7);
    d7 = dot2<K * -6436, K * 2260>(b, dot2<K * -11363, K * 9633>(a, r)) >> OS;
    d5 = dot2<K * -11362, K * 6437>(b, dot2<K * 9633, K * 2261>(a, r)) >> OS;
    d3 = dot2<K * -2259, K * 9633>(b, dot2<K * -6436, K * -11362>(a, r)) >> OS;
    d1 = dot2<K * 9633, K * 11363>(b, dot2<K * 2260, K * 6437>(a, r)) >> OS;
}

// The column pass of jpeg_fdct_islow over two adjacent columns at once: p[v] =
// (row v of column c, row v of column c + 1) as an int16 pair, as one
// ds_read_b32 of the natural-order workspace returns it.  The butterflies and
// the DC/Nyquist sums run as packed 16-bit adds (v_pk_add/sub_u16: every
// partial fits int16 - row outputs lie in [-4096, 4080], so |t10 +- t11| <=
// 32768 - 128 and the +2 of DESCALE stays inside), the rotations as the same
// dot2 chains as fdct8<1, true> per column (operand pairs picked from the
// packed partials by v_perm), and each output row leaves as one int16 pair
// for one ds_write_b32: 8 LDS reads and 8 stores per column pair instead of
// 16 and 16, and half the butterfly VALU.  Equal to fdct8<1> per column.
__device__ __forceinline__ uint32_t pk_add16(uint32_t a, uint32_t b)
{
    uint32_t d;
    asm("v_pk_add_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ uint32_t pk_sub16(uint32_t a, uint32_t b)
{
    uint32_t d;
    asm("v_pk_sub_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ uint32_t pk_sra2(uint32_t a)  // both halves >> 2, arithmetic
{
    uint32_t d;
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(d) : "s"(0x00020002u), "v"(a));
    return d;
}
__device__ __forceinline__ void fdct_col_pair(uint32_t (&p)[8])
{
    const uint32_t t0 = pk_add16(p[0], p[7]), t7 = pk_sub16(p[0], p[7]);
    const uint32_t t1 = pk_add16(p[1], p[6]), t6 = pk_sub16(p[1], p[6]);
    const uint32_t t2 = pk_add16(p[2], p[5]), t5 = pk_sub16(p[2], p[5]);
    const uint32_t t3 = pk_add16(p[3], p[4]), t4 = pk_sub16(p[3], p[4]);
    const uint32_t t10 = pk_add16(t0, t3), t13 = pk_sub16(t0, t3);
    const uint32_t t11 = pk_add16(t1, t2), t12 = pk_sub16(t1, t2);
    uint32_t k2 = 0x00020002u;  // DESCALE(x, PASS1_BITS) rounding, both halves
    asm("" : "+v"(k2));
    const uint32_t t10r = pk_add16(t10, k2);
    p[0] = pk_sra2(pk_add16(t10r, t11));
    p[4] = pk_sra2(pk_sub16(t10r, t11));
    int r = 1 << 15;  // fdct8<1, true>'s rounding constant
    asm("" : "+v"(r));
    int o[2][6];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        // (lo of x, lo of y) or (hi of x, hi of y)
        const uint32_t sel = h ? 0x07060302u : 0x05040100u;
        const uint32_t e = __builtin_amdgcn_perm(t13, t12, sel);
        const uint32_t a = __builtin_amdgcn_perm(t5, t4, sel), b = __builtin_amdgcn_perm(t7, t6, sel);
        o[h][0] = dot2<2 * 9633, 2 * 11363>(b, dot2<2 * 2260, 2 * 6437>(a, r));      // d1
        o[h][1] = dot2<2 * 4433, 2 * 10703>(e, r);                                   // d2
        o[h][2] = dot2<2 * -2259, 2 * 9633>(b, dot2<2 * -6436, 2 * -11362>(a, r));   // d3
        o[h][3] = dot2<2 * -11362, 2 * 6437>(b, dot2<2 * 9633, 2 * 2261>(a, r));     // d5
        o[h][4] = dot2<2 * -10704, 2 * 4433>(e, r);                                  // d6
        o[h][5] = dot2<2 * -6436, 2 * 2260>(b, dot2<2 * -11363, 2 * 9633>(a, r));    // d7
    }
    // each output's value is its int32's high half: (column c, column c + 1)
    constexpr int at[6] = {1, 2, 3, 5, 6, 7};
#pragma unroll
    for (int j = 0; j < 6; j++) p[at[j]] = __builtin_amdgcn_perm((uint32_t)o[1][j], (uint32_t)o[0][j], 0x07060302u);
}

// rgb_ycc_convert (jccolor.c): 16-bit fixed point, FIX(x) = (int)(x*65536+0.5):
//   y  = (19595 r + 38470 g + 7471 b + 32768) >> 16
//   cb = (-11059 r - 21709 g + 32768 b + (128 << 16) + 32767) >> 16
//   cr = (32768 r - 27439 g - 5329 b + (128 << 16) + 32767) >> 16
// Each output's weights sum to a power of two (19595 + 38470 + 7471 = 65536,
// 11059 + 21709 = 27439 + 5329 = 32768), so over e = r - g and d = b - g the
// same integers need two products each and y - 128 (the level-shifted
// sample the DCT takes) one add - exact for every (r, g, b): the multiple of
// 2^16 leaves the floor division unchanged.  Over the negated differences
// (g - r, g - b), packed as int16 pairs, every weight fits int16 (32768 d =
// -32768 * (g - b)): one dot2 per output, the rounding constants (ky, kc,
// held in VGPRs by the caller) as accumulators.
constexpr int YCC_KY = 32768 - (128 << 16), YCC_KC = (128 << 16) + 32767;
__device__ __forceinline__ void rgb_ycc(int r, int g, int b, int ky, int kc, int& y128, int& cb, int& cr)
{
    const uint32_t n = pack16(g - r, g - b);
    y128 = g + (dot2<-19595, -7471>(n, ky) >> 16);
    cb = dot2<11059, -32768>(n, kc) >> 16;
    cr = dot2<-32768, 5329>(n, kc) >> 16;
}
// The same, with Cb and Cr left as an int16 pair (cb, cr): both sums lie in
// [0, 2^24) before the shift, so each sample is its int32's high half - one
// v_perm for the two shifts and the packing.
__device__ __forceinline__ uint32_t rgb_ycc_pk(int r, int g, int b, int ky, int kc, int& y128)
{
    const uint32_t n = pack16(g - r, g - b);
    y128 = g + (dot2<-19595, -7471>(n, ky) >> 16);
    return __builtin_amdgcn_perm((uint32_t)dot2<-32768, 5329>(n, kc), (uint32_t)dot2<11059, -32768>(n, kc), 0x07060302u);
}

// =================================================================== FDCT

// Colour: one workgroup = 16 rows x 256 px = 16 MCUs of one MCU row (96 blocks);
// every phase has 1-3 equal tasks per thread.  LDS 20.4 KiB; three tiles per
// workgroup at 74 VGPRs -> 6 workgroups/CU.
//   B. one row pair x 8 px per thread straight from HBM (24 B runs; a wave
//      reads four contiguous 768 B row pieces; edges clamped): YCbCr, two Y
//      row-DCTs in registers -> workspace; h2v2_downsample of its own 2x8
//      Cb/Cr (bias 1,2,..) -> 4 + 4 bytes of the downsampled chroma tile
//   C. chroma row-DCT, one row task per thread (bottom rows past the image
//      replicate the last chroma row, jcprepct.c expand_bottom_edge)
//   D. column DCT, 3 column tasks per thread into registers; barrier; zig-zag
//      scatter over the (now dead) workspace
//   E. dummy blocks (jccoefct.c) + 8-B stores into the interleaved layout
// The workspace stride of 68 int16 (34 dwords) puts consecutive blocks on
// distinct LDS banks for every access pattern above.
constexpr int FDC_MCU = 16;           // MCUs per colour tile
constexpr int FDC_PX = FDC_MCU * 16;  // 256 px
constexpr int FDC_BLK = FDC_MCU * 6;  // 96 blocks
constexpr int WSTR = 72;              // workspace int16 per block (row-pass writes, column reads and
                                      // the natural-order output of phase D are LDS-bank-conflict-free)

// One row of a block (8 int16, 16-B aligned: WSTR * 2 = 144 B per block) as
// one ds_write_b128: its 8-lane groups put the eight blocks of a phase-B row
// on distinct banks, where two ds_write_b64 (16-lane groups) were 2-way
// conflicted (phase B's rows r and r + 2 of one group are 8 dwords apart,
// as are blocks 6 apart).
#ifndef ICX_FDCT_ST128
#define ICX_FDCT_ST128 1
#endif
__device__ __forceinline__ void st_row8(int16_t* p, const int (&v)[8])
{
    if (ICX_FDCT_ST128) {
        *(uint4*)p = make_uint4(pack16(v[0], v[1]), pack16(v[2], v[3]), pack16(v[4], v[5]), pack16(v[6], v[7]));
    } else {
        *(uint2*)p = make_uint2(pack16(v[0], v[1]), pack16(v[2], v[3]));  // one v_perm per pair
        *(uint2*)(p + 4) = make_uint2(pack16(v[4], v[5]), pack16(v[6], v[7]));
    }
}

// Phase B loads: this thread's rows 2i, 2i+1 of the tile, pixels 8sg..8sg+7
// (24 bytes each), edges clamped.  Separate from the arithmetic so the kernel
// can issue the next tile's loads before it computes the current one.
#ifndef ICX_FDCT_NOHOIST
#define ICX_FDCT_NOHOIST 1
#endif
// tile / tiles_x by one scalar multiply-high (a 32-bit division is ~30
// scalar instructions in front of every tile)
__device__ __forceinline__ int fdct_tile_row(const ImgDesc& D, int tile)
{
    return D.tiles_xm ? (int)__umulhi((uint32_t)tile, D.tiles_xm) : tile;
}

struct FdctTile {
    const ImgDesc* D;
    int img, tx, my;
};

__device__ __forceinline__ FdctTile fdct_tile(const ImgDesc* __restrict__ descs, const int32_t* __restrict__ ids,
                                              const int64_t* __restrict__ prefix, int m, int64_t item)
{
    // 2-D launch (every image of the plan has as many tiles): slot = y, item = tile
    const int slot = gridDim.y > 1 ? (int)blockIdx.y : find_slot(prefix, m, item);
    const int img = ids ? ids[slot] : slot;
    const ImgDesc* D = &descs[img];
    const int tile = gridDim.y > 1 ? (int)item : (int)(item - prefix[slot]);
    const int my = fdct_tile_row(*D, tile);
    return FdctTile{D, img, tile - my * (int)D->tiles_x, my};
}

// Wave-local tiles (ICX_FDCT_WAVE): wave w of the workgroup owns MCUs 4w..4w+3
// of the tile (pixels 64w..64w+63, blocks 24w..24w+23, its own list region and
// stage) in every phase, so the phases hand over with wave barriers only and
// the four waves never wait for one another.  Lane = (row pair i, 8-px group):
// i = lane >> 3, sg = 8w + (lane & 7).  Otherwise a phase spans the tile:
// i = t >> 5, sg = t & 31, with workgroup barriers between phases.
// Measured (scripts/ab.sh, 300 4K frames, 3 rounds): FDCT -1.0 % against the
// tile-wide phases (profiles/r3/ab_r3y_fdct_wave.txt).
#ifndef ICX_FDCT_WAVE
#define ICX_FDCT_WAVE 1
#endif
constexpr bool FDCT_WAVE = ICX_FDCT_WAVE != 0;
// Column DCT of two thirds of a wave's blocks on packed column pairs
// (fdct_col_pair), the rest one column per lane.
#ifndef ICX_FDCT_PKCOL
#define ICX_FDCT_PKCOL 1
#endif
// Phase B: each pixel's Cb, Cr as one int16 pair (rgb_ycc_pk), the 2x2 sums
// and the h2v2 bias as packed adds, the downsampled bytes by v_perm.
#ifndef ICX_FDCT_PKSUM
#define ICX_FDCT_PKSUM 1
#endif
__device__ __forceinline__ int fdct_row_pair(int t) { return FDCT_WAVE ? (t & 63) >> 3 : t >> 5; }
__device__ __forceinline__ int fdct_px_group(int t) { return FDCT_WAVE ? ((t >> 6) << 3) | (t & 7) : t & 31; }
// the hand-over between two phases of a tile
__device__ __forceinline__ void fdct_phase_sync()
{
    if (FDCT_WAVE)
        __builtin_amdgcn_wave_barrier();
    else
        __syncthreads();
}

__device__ __forceinline__ void fdct_load(const FdctTile& T, uint32_t (&wv)[2][6])
{
    const ImgDesc& D = *T.D;
    const int t = threadIdx.x, i = fdct_row_pair(t), sg = fdct_px_group(t);
    const int W = D.w, H = D.h, x0 = T.tx * FDC_PX, y0 = T.my * 16;
    const uint8_t* px = D.px;
    const bool fast = (x0 + FDC_PX <= W) && (((uintptr_t)px & 7) == 0) && ((D.stride & 7) == 0);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int y = min(y0 + 2 * i + h, H - 1);
        const uint8_t* row = px + (size_t)y * D.stride;
#if ICX_FDCT_STATIC
        {
            // the three loads on every path (an edge tile reads 24 aligned
            // bytes at the start of the image's allocation instead, then
            // assembles its pixels below): a value merged from two branches
            // costs a copy, and the copy waits for the load at once
            const uint8_t* p = fast ? row + (size_t)(x0 + sg * 8) * 3 : (const uint8_t*)((uintptr_t)px & ~(uintptr_t)7);
            const int2 a = ld8(p), b = ld8(p + 8), c = ld8(p + 16);
            wv[h][0] = a.x; wv[h][1] = a.y; wv[h][2] = b.x;
            wv[h][3] = b.y; wv[h][4] = c.x; wv[h][5] = c.y;
        }
        if (!fast) {
#else
        if (fast) {
            const uint8_t* p = row + (size_t)(x0 + sg * 8) * 3;
            const int2 a = ld8(p), b = ld8(p + 8), c = ld8(p + 16);
            wv[h][0] = a.x; wv[h][1] = a.y; wv[h][2] = b.x;
            wv[h][3] = b.y; wv[h][4] = c.x; wv[h][5] = c.y;
        } else {
#endif
            const GAS uint8_t* g = gp(row);
            // opaque here, so the compiler does not hoist this path's eight
            // clamped pixel offsets in front of the (wave-uniform) branch
            int xb = x0 + sg * 8;
#if ICX_FDCT_NOHOIST
            asm volatile("" : "+v"(xb));
#endif
#pragma unroll
            for (int k = 0; k < 6; k++) wv[h][k] = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int sx = min(xb + k, W - 1);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int o = 3 * k + c;
                    wv[h][o >> 2] |= (uint32_t)g[(size_t)sx * 3 + c] << ((o & 3) * 8);
                }
            }
        }
    }
}

// Candidate lists of one FDCT tile (nblk scan blocks from bbase; the tile's
// list region starts at entry `base`, COEF_SLOTS entries reserved per block).
// oz[blk] holds block blk's raw coefficients in natural order (fix(blk, lane,
// c) applies dummy blocks; lane = zig-zag index reads position c_zz_to_nat[lane]).  The DC and every AC coefficient with |c| >= thr
// (lane 0's thr is negative; the others hold the smallest quantiser
// threshold of k over the qualities this image may be coded at) form the
// block's list, entries float_bits(c) | (chroma << 9) | (k << 3) in k order, padded to a
// multiple of 4 entries (k_huff reads 16-B groups; the padding holds whatever
// the stage held - k_huff codes only the first `length` entries).
// One wave per group of STEP blocks (one MCU for colour; luma(a): block
// blk0 + a is luma), lane = k: per block a ballot/mbcnt partition
// (candidates first, then the rest) into the wave's LDS stage, the group's
// lists back to back; then the group leaves as 16-B pieces into the group's
// own reserved region.  No cross-wave scan: lists are packed per group.
// Lengths and offsets go to L.meta and, after the caller's barrier, to
// ncoef / coff (store_list_meta).
// Phase-E LDS of a tile: one stage per wave for its group's lists, 64 dwords
// the lanes with nothing to store write to (never read, shared by the waves,
// so the stores need no exec mask), and per block (offset in its group << 7)
// | list length.
#ifndef ICX_FDCT_STATIC
#define ICX_FDCT_STATIC 1  // k_fdct_color: loads and stores the compiler can count on every path (below); FDCT -2 % (ab_r5ao_fdct_static.txt)
#endif
#ifndef ICX_FDCT_EMIT_LA
#define ICX_FDCT_EMIT_LA 1
#endif
template <int NB, int STEP>
struct ListStage {
    uint32_t st[4][STEP * 64];
    uint32_t dummy[64];  // follows st[3]: index 4 * STEP * 64 + lane
    uint16_t meta[NB];
};

// v_writelane: lane `a` (0..7, a constant once the caller's loop is unrolled)
// of v takes the wave-uniform value x - one VALU op, no lane compare.
#define ICX_WRITELANE(A) \
    case A: asm volatile("v_writelane_b32 %0, %1, " #A : "+v"(v) : "s"(x)); break;
__device__ __forceinline__ int writelane(int v, int x, int a)
{
    switch (a) {
        ICX_WRITELANE(0) ICX_WRITELANE(1) ICX_WRITELANE(2) ICX_WRITELANE(3)
        ICX_WRITELANE(4) ICX_WRITELANE(5) ICX_WRITELANE(6) ICX_WRITELANE(7)
    }
    return v;
}
#undef ICX_WRITELANE

template <int NB, int STEP, bool FULL, class Fix, class Luma>
__device__ __forceinline__ uint32_t emit_lists(const ImgDesc& D, int64_t base, int nblk, int16_t (*oz)[WSTR],
                                               ListStage<NB, STEP>& L, const float (&thr)[2], Fix fix, Luma luma,
                                               int nat_in = -1)
{
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    uint32_t* st = L.st[wave];
    uint32_t* const st0 = &L.st[0][0];
    const int dummy_at = 4 * STEP * 64 + lane;  // L.dummy[lane] as an index into st0
    uint32_t total = 0;
    // oz holds natural order; lane = zig-zag index (nat_in: the caller's copy,
    // loaded once per workgroup - a vector load here, behind the next tile's
    // pixel loads, would wait for them)
    const int nat = nat_in >= 0 ? nat_in : c_zz_to_nat[lane];
    // wave w takes groups NB/(4 STEP) * w .. (consecutive blocks) and packs their
    // lists back to back in its own region: one partly used cache line per wave
    // region instead of one per group (k_huff's gathers fetch whole lines)
    constexpr int GPW = NB / (4 * STEP);  // groups per wave
    GAS u32x4_t* const region = (GAS u32x4_t*)(D.coefs + base + (int64_t)wave * GPW * STEP * COEF_SLOTS);
#if ICX_FDCT_STATIC
    // every group runs (one store each, on every path: see the stores below);
    // a group past the tile's last block codes nothing (run = 0)
#pragma unroll
#endif
    for (int g = 0; g < GPW; g++) {
        const int blk0 = (wave * GPW + g) * STEP;
#if ICX_FDCT_STATIC
        const bool live = blk0 < nblk;  // wave-uniform
#else
        if (blk0 >= nblk) break;
#endif
        int c[STEP];
#pragma unroll
        for (int a = 0; a < STEP; a++)
            c[a] = FULL || blk0 + a < nblk ? fix(blk0 + a, lane, (int)oz[blk0 + a][nat]) : 0;
        // run: padded entries of the group so far (wave-uniform); lane a < STEP of
        // meta: block a's (offset in the wave region, 16-B units) << 7 | length
        int run = 0, meta = 0;
#pragma unroll
        for (int a = 0; a < STEP; a++) {
            if (!FULL && blk0 + a >= nblk) break;  // wave-uniform (partial grey tiles)
            const float cf = (float)c[a];
            const bool cand = fabsf(cf) >= (luma(a) ? thr[0] : thr[1]);
            const uint64_t mask = __ballot(cand);
            const int cnt = __builtin_amdgcn_readfirstlane(__popcll(mask)), r4 = (cnt + 3) & ~3;
            // the candidate's stage index: wave base + run + candidates below the lane
            // the padding to a whole 16-B group is left as it is in the stage:
            // k_huff never codes an entry past the list's length (writing the
            // block's first non-candidates there cost 4 VALU per block: FDCT +9 %)
            // one v_cndmask on the ballot: as a C select the compiler branches
            // around the candidate address (exec save / restore: SALU)
            const uint32_t ent_v = __float_as_uint(cf) | ((uint32_t)lane << 3) | (luma(a) ? 0u : 0x200u);
            if (ICX_FDCT_EMIT_LA) {
                // byte address: candidates below the lane counted from 0 (no
                // move of the wave-uniform base into a VGPR), then one
                // v_lshl_add_u32 with the scalar byte base
                const uint32_t below =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const uint32_t at_b = below * 4u + (uint32_t)(wave * (STEP * 64) + run) * 4u;
                uint32_t addr;
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(addr) : "v"(dummy_at * 4), "v"(at_b), "s"(mask));
                *(uint32_t*)((char*)st0 + addr) = ent_v;
            } else {
                const int at = (int)__builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, (uint32_t)(wave * (STEP * 64) + run)));
                int idx;
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(idx) : "v"(dummy_at), "v"(at), "s"(mask));
                st0[idx] = ent_v;
            }
            // total + run is a multiple of 4: (x >> 2) << 7 = x << 5
            meta = writelane(meta, (((int)total + run) << 5) | cnt, a);  // scalar arithmetic, one VALU op
            run += r4;
        }
#if ICX_FDCT_STATIC
        run = live ? run : 0;
#endif
        if (lane < STEP && blk0 + lane < nblk) L.meta[blk0 + lane] = (uint16_t)meta;
        __builtin_amdgcn_wave_barrier();
        GAS u32x4_t* dst = region + total / 4;
#if ICX_FDCT_STATIC
        {
            // one store per lane whatever the lists' length (lanes past the
            // group's last 16-B piece store that piece again: same address,
            // same bytes; an empty group stores stage garbage at the group's
            // start, inside the region and past every list that k_huff codes),
            // so the stores are one instruction the compiler counts on every
            // path (see k_fdct_color); a group of more than 256 entries stores
            // the rest and then waits for its stores (rare: noise content)
            const int n4 = run / 4;
            const int p = lane < n4 ? lane : n4 > 0 ? n4 - 1 : 0;
            const uint4 v = *(const uint4*)&st[4 * p];
            u32x4_t w;
            w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
            dst[p] = w;
            // (a second store per lane on every path instead of this branch:
            // FDCT +1 %, ab_r5as_fdct_two_stores.txt)
            if (n4 > 64) {
                for (int q = lane + 64; q < n4; q += 64) {
                    const uint4 v2 = *(const uint4*)&st[4 * q];
                    u32x4_t w2;
                    w2.x = v2.x; w2.y = v2.y; w2.z = v2.z; w2.w = v2.w;
                    dst[q] = w2;
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            }
        }
#else
        for (int p = lane; p < run / 4; p += 64) {
            const uint4 v = *(const uint4*)&st[4 * p];
            u32x4_t w;
            w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
            dst[p] = w;
        }
#endif
        total += run;
        __builtin_amdgcn_wave_barrier();
    }
    return total;  // wave-uniform: the caller credits it to the image's counter
}

// After the barrier that ends emit_lists: lengths and 16-B-unit offsets.
template <int NB, int STEP, bool WAVE = false>
__device__ __forceinline__ void store_list_meta(const ImgDesc& D, int64_t base, uint32_t bbase, int nblk,
                                                const ListStage<NB, STEP>& L)
{
    constexpr int GPW = NB / (4 * STEP);
    // WAVE: after a wave barrier, each wave stores the meta of its own blocks
#if ICX_FDCT_STATIC
    if (WAVE) {
        // every lane stores (the compiler counts the stores on every path):
        // a lane without a block of its own stores its wave's last block
        // again, the same bytes to the same address.  A wave with no block in
        // this (edge) tile owns nothing it could repeat - the tile's last
        // block is another wave's, whose meta it may read before the owner
        // writes it (no barrier between waves) - so its lanes store to the
        // image's dummy slot past the padded block arrays (never read).
        const int w0 = (int)(threadIdx.x >> 6) * (GPW * STEP);
        const bool dead = w0 >= nblk;  // wave-uniform
        const int lim = min(w0 + GPW * STEP, nblk) - 1;
        int t = w0 + (int)(threadIdx.x & 63);
        t = dead ? w0 : t < lim ? t : lim;
        const uint32_t m = L.meta[t];  // (a dead wave reads its own stale entry: unused)
        const uint32_t at = dead ? (uint32_t)D.nchunks * CHUNK_BLOCKS : bbase + (uint32_t)t;
        // global, not flat, stores: a flat store counts on the LDS counter too,
        // and the next tile's LDS waits would wait for it
        gp(D.ncoef)[at] = (uint8_t)(m & 127);
        gp(D.coff)[at] = (uint32_t)((base + (t / (GPW * STEP)) * (GPW * STEP * COEF_SLOTS)) >> 2) + (m >> 7);
        return;
    }
#endif
    const int t = WAVE ? (threadIdx.x >> 6) * (GPW * STEP) + (threadIdx.x & 63) : threadIdx.x;
    if ((!WAVE || (threadIdx.x & 63) < GPW * STEP) && t < nblk) {
        const uint32_t m = L.meta[t];
        D.ncoef[bbase + t] = (uint8_t)(m & 127);
        D.coff[bbase + t] = (uint32_t)((base + (t / (GPW * STEP)) * (GPW * STEP * COEF_SLOTS)) >> 2) + (m >> 7);
    }
}

// Phases B (arithmetic) .. E of one tile; LDS is free again on return.
template <bool BGR>
__device__ __forceinline__ uint32_t fdct_compute(const FdctTile& T, const uint32_t (&wv)[2][6],
                                             const QNode* __restrict__ nodes, ImgState* states,
                                             uint8_t (*cds)[8][FDC_PX / 2], int16_t (*ws)[WSTR],
                                             ListStage<FDC_BLK, 6>& L, int nat = -1, const float* thr_in = nullptr)
{
    const ImgDesc& D = *T.D;
    const int tx = T.tx, my = T.my;
    const int H = D.h;
    const int t = threadIdx.x;
    int16_t (*oz)[WSTR] = ws;     // natural-order output (phase D)
    const QNode& CN = nodes[D.cand_node];
    const float thr[2] = {(t & 63) ? (thr_in ? thr_in[0] : CN.qf[0][t & 63].x) : -1.0f,
                          (t & 63) ? (thr_in ? thr_in[1] : CN.qf[1][t & 63].x) : -1.0f};
    const int crows = (H + 1) >> 1;             // chroma rows with image data
    const bool tail = crows - my * 8 < 8;       // ... ending inside this tile (workgroup-uniform)

    // wave-local tiles stage a tail tile's downsampled chroma in the wave's own
    // list stage (free until phase E): [comp][chroma row][its 32 columns]
    uint8_t (*const cdw)[8][32] = (uint8_t (*)[8][32])&L.st[t >> 6][0];

    // ---- B: YCbCr, two Y row-DCTs, h2v2_downsample of this thread's 2x8 chroma
    // (+ C: the chroma row DCTs, except in tail tiles)
    {
        const int i = fdct_row_pair(t), sg = fdct_px_group(t);
        int csum[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // 2x2 sums of Cb, Cr
        uint32_t psum[4];                               // ICX_FDCT_PKSUM: the same as (Cb, Cr) pairs
        int ky = YCC_KY, kc = YCC_KC;
        asm("" : "+v"(ky), "+v"(kc));
#pragma unroll
        for (int h = 0; h < 2; h++) {
            int yv[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int o0 = 3 * k, o1 = 3 * k + 1, o2 = 3 * k + 2;
                const int c0 = (wv[h][o0 >> 2] >> ((o0 & 3) * 8)) & 255;
                const int c1 = (wv[h][o1 >> 2] >> ((o1 & 3) * 8)) & 255;
                const int c2 = (wv[h][o2 >> 2] >> ((o2 & 3) * 8)) & 255;
                const int R = BGR ? c2 : c0, G = c1, B = BGR ? c0 : c2;
                if (ICX_FDCT_PKSUM) {
                    const uint32_t cc = rgb_ycc_pk(R, G, B, ky, kc, yv[k]);
                    // the h2v2 bias (1, 2, 1, 2 by output column) rides on the
                    // group's first pair: sums stay < 2^10 per half
                    psum[k >> 1] = pk_add16(h == 0 && !(k & 1) ? (((k >> 1) & 1) ? 0x00020002u : 0x00010001u)
                                                               : psum[k >> 1], cc);
                } else {
                    int cb, cr;
                    rgb_ycc(R, G, B, ky, kc, yv[k], cb, cr);
                    csum[0][k >> 1] += cb;
                    csum[1][k >> 1] += cr;
                }
            }
            fdct8<0>(yv[0], yv[1], yv[2], yv[3], yv[4], yv[5], yv[6], yv[7]);
            const int r = 2 * i + h;
            const int blk = (sg >> 1) * 6 + (r >> 3) * 2 + (sg & 1);
            st_row8(&ws[blk][(r & 7) * 8], yv);
        }
        uint32_t w[2];
        if (ICX_FDCT_PKSUM) {
            uint32_t q[4];
#pragma unroll
            for (int j = 0; j < 4; j++) asm("v_pk_lshrrev_b16 %0, %1, %2" : "=v"(q[j]) : "s"(0x00020002u), "v"(psum[j]));
            // (cb_j, cr_j) halves -> (cb0 cb1 cr0 cr1), (cb2 cb3 cr2 cr3) -> Cb word, Cr word
            const uint32_t x01 = __builtin_amdgcn_perm(q[1], q[0], 0x06020400u);
            const uint32_t x23 = __builtin_amdgcn_perm(q[3], q[2], 0x06020400u);
            w[0] = __builtin_amdgcn_perm(x23, x01, 0x05040100u);
            w[1] = __builtin_amdgcn_perm(x23, x01, 0x07060302u);
        } else {
#pragma unroll
            for (int c = 0; c < 2; c++) {  // h2v2_downsample: bias 1, 2, 1, 2 by output column
                w[c] = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) w[c] |= (uint32_t)((csum[c][j] + 1 + (j & 1)) >> 2) << (8 * j);
            }
        }
        if (!tail) {
            // C, fused: chroma row i of chroma block sg >> 1 is 4 + 4 samples of
            // this lane and its neighbour (lanes 2k, 2k + 1).  The pair swaps
            // one word by DPP (quad_perm 1,0,3,2): the even lane then holds the
            // block row's 8 Cb samples, the odd lane its 8 Cr samples - one
            // chroma row DCT per thread, no LDS round trip, one barrier less.
            const int comp = sg & 1;
            const uint32_t recv = (uint32_t)__builtin_amdgcn_mov_dpp((int)(comp ? w[0] : w[1]), 0xB1, 0xF, 0xF, false);
            const uint32_t lo = comp ? recv : w[0], hi = comp ? w[1] : recv;
            int v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = (int)(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 255) - 128;
            fdct8<0>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
            st_row8(&ws[(sg >> 1) * 6 + 4 + comp][i * 8], v);
        } else if (FDCT_WAVE) {
#pragma unroll
            for (int c = 0; c < 2; c++) *(uint32_t*)&cdw[c][i][(sg & 7) * 4] = w[c];
        } else {
#pragma unroll
            for (int c = 0; c < 2; c++) *(uint32_t*)&cds[c][i][sg * 4] = w[c];
        }
    }
    fdct_phase_sync();

    // ---- C (bottom tiles whose chroma rows end inside the tile): the rows
    // past the image replicate the last chroma row (jcprepct.c
    // expand_bottom_edge), by index from the staged samples; 256 row tasks
    // (wave-local: the wave's 4 chroma blocks x 2 components x 8 rows)
    if (tail) {
        const int comp = FDCT_WAVE ? (t >> 5) & 1 : t >> 7, cr = (t >> (FDCT_WAVE ? 2 : 4)) & 7;
        const int cb = FDCT_WAVE ? ((t >> 6) << 2) | (t & 3) : t & 15;
        const int re = min(cr, crows - 1 - my * 8);
        const uint2 u = FDCT_WAVE ? *(const uint2*)&cdw[comp][re][(t & 3) * 8] : *(const uint2*)&cds[comp][re][cb * 8];
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = (int)(((j < 4 ? u.x : u.y) >> (8 * (j & 3))) & 255) - 128;
        fdct8<0>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        st_row8(&ws[cb * 6 + 4 + comp][cr * 8], v);
        fdct_phase_sync();
    }

    // ---- D: column DCT, 3 tasks per thread, in place: the thread of (block,
    // column) is the only reader and writer of that column, so the natural-
    // order output needs no barrier between the reads and the writes
    // (wave-local: wave w's 24 blocks)
#if ICX_FDCT_PKCOL
    if (FDCT_WAVE) {
        // wave-local: blocks 0..15 of the wave as column pairs (lane = block *
        // 4 + pair: a ds_read_b32 row of 32 lanes covers 8 blocks x 4 pairs on
        // distinct banks), blocks 16..23 one column per lane
        {
            const int blk = (t >> 6) * 24 + ((t & 63) >> 2), c = (t & 3) * 2;
            uint32_t p[8];
#pragma unroll
            for (int v = 0; v < 8; v++) p[v] = *(const uint32_t*)&ws[blk][v * 8 + c];
            fdct_col_pair(p);
#pragma unroll
            for (int v = 0; v < 8; v++) *(uint32_t*)&oz[blk][v * 8 + c] = p[v];
        }
        {
            // even columns on lanes 0..31, odd ones on 32..63: the two lanes
            // of one dword (columns 2c, 2c + 1) sit in different halves of
            // the wave, so neither the reads nor the 16-bit stores conflict
            const int blk = (t >> 6) * 24 + 16 + ((t >> 2) & 7), col = ((t & 3) << 1) | ((t >> 5) & 1);
            int32_t d[8];
#pragma unroll
            for (int v = 0; v < 8; v++) d[v] = ws[blk][v * 8 + col];
            fdct8<1, true>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#pragma unroll
            for (int v = 0; v < 8; v++) oz[blk][v * 8 + col] = (int16_t)(d[v] >> 16);  // ds_write_b16_d16_hi
        }
    } else
#endif
    {
        const int col = t & 7;
#pragma unroll
        for (int rep = 0; rep < 3; rep++) {
            const int blk = FDCT_WAVE ? (t >> 6) * 24 + ((t & 63) >> 3) + 8 * rep : (t >> 3) + 32 * rep;
            int32_t d[8];
#pragma unroll
            for (int v = 0; v < 8; v++) d[v] = ws[blk][v * 8 + col];
            fdct8<1, true>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#pragma unroll
            for (int v = 0; v < 8; v++) oz[blk][v * 8 + col] = (int16_t)(d[v] >> 16);  // ds_write_b16_d16_hi
        }
    }
    fdct_phase_sync();

    // ---- E: dummy blocks + candidate lists.  jccoefct.c compress_data: a Y
    // block right of ceil(W/8) or below ceil(H/8) gets AC = 0 and the DC of
    // MCU_buffer[blkn-1] (right edge) or of the last block of the MCU's previous
    // block row (bottom).  One wave per block, lane = zig-zag index: the lanes
    // whose coefficient can be nonzero in some trial (and lane 0, the DC) are
    // compacted by ballot/mbcnt into the block's list.
    const int nmcu = min(FDC_MCU, D.mcux - tx * FDC_MCU);
    const int nblk = nmcu * 6;
    const bool bottom = (2 * my + 1) >= D.yhb;
    const uint32_t bbase = (uint32_t)(my * D.mcux + tx * FDC_MCU) * 6;  // < 2^31 blocks per image
    const bool plain = nmcu == FDC_MCU && !bottom && 2 * (tx * FDC_MCU + FDC_MCU - 1) + 1 < D.ywb;
    auto fix = [&](int blk, int lane, int c) -> int {
        if (!plain) {
            const int mcu = blk / 6, yb = blk - mcu * 6;
            const bool right = (2 * (tx * FDC_MCU + mcu) + 1) >= D.ywb;
            if (yb < 4 && ((yb >= 2 && bottom) || ((yb & 1) && right))) {  // dummy block (wave-uniform)
                // effective source: right dummy in row 0 -> block 0; bottom row -> eff(block 1);
                // right dummy in row 1 (not bottom) -> block 2 (a DC never moves in compaction)
                const int src = yb == 1 ? 0 : bottom ? (right ? 0 : 1) : 2;
                c = lane == 0 ? oz[mcu * 6 + src][0] : 0;
            }
        }
        return c;
    };
    const int64_t tile_id = (int64_t)my * D.tiles_x + tx;
    const int64_t base = tile_id * (FDC_BLK * COEF_SLOTS);
    auto luma = [](int a) { return a < 4; };  // one MCU per step: Y0 Y1 Y2 Y3 Cb Cr
    uint32_t entries;
    if (plain)  // interior tile: no dummy blocks
        entries = emit_lists<FDC_BLK, 6, true>(D, base, nblk, oz, L, thr, [](int, int, int c) { return c; }, luma, nat);
    else
        entries = emit_lists<FDC_BLK, 6, true>(D, base, nblk, oz, L, thr, fix, luma, nat);
    fdct_phase_sync();
    store_list_meta<FDC_BLK, 6, FDCT_WAVE>(D, base, bbase, nblk, L);
    // LDS free for the next tile (wave-local: the wave's next phase B writes
    // only its own blocks and stage, after its own reads above)
#if !ICX_FDCT_NOTAIL
    if (!FDCT_WAVE) __syncthreads();
#endif
    return entries;
}

// The FDCT keeps no count of the list entries it writes: the byte
// accounting (profiling only) and the probe bound get them from
// k_list_count.  A global atomic
// per wave and tile (16 counters per image) cost 5.7 % of the FDCT time, one
// per workgroup still 4.3 % (profiles/r3/ab_r3zg_fdct_lds.txt,
// ab_r3zh_fdct_ent.txt): a wave whose last instruction is a device-scope
// atomic holds its slot for the atomic's round trip.

// FDCT_TILES consecutive tiles per workgroup, software-pipelined: the next
// tile's pixel loads are issued before the current tile is computed, so each
// CU keeps more bytes in flight than one tile's phase B alone would.
// Measured (300 4K frames): T = 1 6.65-6.81 ms, T = 2 6.29-6.33 ms, T = 4
// 6.39-6.46 ms (round 1).  Round 3, after the packed column pass and the
// multiply-high tile row: T = 3 (74 VGPRs, 6 waves/SIMD) -2.1 % against T = 2
// (54 VGPRs, 8 waves/SIMD), T = 4 +1.1 % (profiles/r3/ab_r3ze_fdct_tiles.txt,
// 5 interleaved rounds): three tiles' worth of pixel loads in flight per
// workgroup hide more than the two extra waves per SIMD did.
#ifndef ICX_FDCT_TILES
#define ICX_FDCT_TILES 3
#endif
constexpr int FDCT_TILES = ICX_FDCT_TILES;

template <bool BGR>
__global__ __launch_bounds__(256) void k_fdct_color(const ImgDesc* __restrict__ descs,
                                                    const QNode* __restrict__ nodes, ImgState* states,
                                                    const int32_t* __restrict__ ids,
                                                    const int64_t* __restrict__ prefix, int m)
{
    // 13.5 KiB row-pass output / coefficients + 6.4 KiB shared by the
    // downsampled chroma (phases B, C) and the list stages (phase E): 20416 B
    // (room for eight workgroups per CU; the VGPRs of three pipelined tiles
    // allow six)
    __shared__ __attribute__((aligned(16))) int16_t ws[FDC_BLK][WSTR];
    __shared__ __attribute__((aligned(16))) union {
        uint8_t cds[2][8][FDC_PX / 2];
        ListStage<FDC_BLK, 6> ls;
    } u;
    const int64_t total = gridDim.y > 1 ? prefix[1] - prefix[0] : prefix[m];  // items of this launch row
    const int64_t item0 = (int64_t)blockIdx.x * FDCT_TILES;
#if ICX_FDCT_STATIC
    // Each tile's pixels in registers of their own, the next tile's loads
    // issued before this tile is computed - unconditionally (a launch's last
    // workgroup loads its last tile again instead of branching around the
    // loads), and no register copies between tiles (a copy of a load's
    // destination waits for the load).  With the list and meta stores one
    // instruction each on every path, the compiler's wait for the next tile's
    // pixels leaves this tile's stores in flight (vector-memory counters count
    // stores too, in order: a store it cannot count on every path is waited
    // for).
    const int nat = c_zz_to_nat[threadIdx.x & 63];  // emit_lists' gather index, ahead of every pixel load
    uint32_t px[FDCT_TILES][2][6];
    float thr[FDCT_TILES][2];  // the tile's candidate thresholds (fdct_compute), loaded with its pixels
    FdctTile tl[FDCT_TILES];
    auto fetch = [&](int k, int64_t item) {
        tl[k] = fdct_tile(descs, ids, prefix, m, item);
        fdct_load(tl[k], px[k]);
        // raw values, lane 0's replaced where they are used: a select here
        // would wait for the loads at once
        const QNode& CN = nodes[tl[k].D->cand_node];
        thr[k][0] = CN.qf[0][threadIdx.x & 63].x;
        thr[k][1] = CN.qf[1][threadIdx.x & 63].x;
    };
    fetch(0, item0);
#pragma unroll
    for (int k = 0; k < FDCT_TILES; k++) {
        if (k > 0 && item0 + k >= total) break;  // workgroup-uniform
        if (k + 1 < FDCT_TILES) fetch(k + 1 < FDCT_TILES ? k + 1 : 0, min(item0 + k + 1, total - 1));
        fdct_compute<BGR>(tl[k], px[k], nodes, states, u.cds, ws, u.ls, nat, thr[k]);
    }
#else
    uint32_t cur[2][6], nxt[2][6];
    FdctTile tc = fdct_tile(descs, ids, prefix, m, item0);
    fdct_load(tc, cur);
#pragma unroll
    for (int k = 0; k < FDCT_TILES; k++) {
        FdctTile tn = tc;
        const bool more = k + 1 < FDCT_TILES && item0 + k + 1 < total;
        if (more) {
            tn = fdct_tile(descs, ids, prefix, m, item0 + k + 1);
            fdct_load(tn, nxt);
        }
        fdct_compute<BGR>(tc, cur, nodes, states, u.cds, ws, u.ls);
        if (!more) break;
        tc = tn;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < 6; q++) cur[h][q] = nxt[h][q];
    }
#endif
}

// Grey (1 component, non-interleaved): one workgroup = 8 rows x 128 px = 16 blocks.
__global__ __launch_bounds__(256) void k_fdct_gray(const ImgDesc* __restrict__ descs,
                                                   const QNode* __restrict__ nodes, ImgState* states,
                                                   const int32_t* __restrict__ ids,
                                                   const int64_t* __restrict__ prefix, int m)
{
    __shared__ __attribute__((aligned(16))) int32_t ws[16][64];
    __shared__ __attribute__((aligned(16))) int16_t oz[16][WSTR];
    __shared__ __attribute__((aligned(16))) ListStage<16, 4> ls;
    // 2-D launch (every image of the plan has as many tiles): slot = y
    const int slot = gridDim.y > 1 ? (int)blockIdx.y : find_slot(prefix, m, blockIdx.x);
    const int img = ids ? ids[slot] : slot;
    const ImgDesc& D = descs[img];
    const int tile = gridDim.y > 1 ? (int)blockIdx.x : (int)(blockIdx.x - prefix[slot]);
    const int by = fdct_tile_row(D, tile), tx = tile - by * (int)D.tiles_x;
    const int W = D.w, H = D.h, x0 = tx * 128;
    const int t = threadIdx.x;
    if (t < 128) {
        const int r = t >> 4, s = t & 15;
        const int y = min(by * 8 + r, H - 1);
        const GAS uint8_t* row = gp(D.px + (size_t)y * D.stride);
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (int)row[min(x0 + s * 8 + k, W - 1)] - 128;
        fdct8<0>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        int32_t* dst = &ws[s][r * 8];
        *(int4*)dst = make_int4(v[0], v[1], v[2], v[3]);
        *(int4*)(dst + 4) = make_int4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    if (t < 128) {
        const int blk = t >> 3, col = t & 7;
        int32_t d[8];
#pragma unroll
        for (int v = 0; v < 8; v++) d[v] = ws[blk][v * 8 + col];
        fdct8<1, true>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#pragma unroll
        for (int v = 0; v < 8; v++) oz[blk][v * 8 + col] = (int16_t)(d[v] >> 16);  // ds_write_b16_d16_hi
    }
    __syncthreads();
    const int nblk = min(16, D.mcux - tx * 16);
    const uint32_t bbase = (uint32_t)by * D.mcux + tx * 16;
    const float thr[2] = {(t & 63) ? nodes[D.cand_node].qf[0][t & 63].x : -1.0f, 0.0f};
    const int64_t base = (int64_t)tile * (16 * COEF_SLOTS);
    emit_lists<16, 4, false>(D, base, nblk, oz, ls, thr, [](int, int, int c) { return c; }, [](int) { return true; });
    __syncthreads();
    store_list_meta(D, base, bbase, nblk, ls);
}

// Candidate-list entries an FDCT wrote for each image of a plan (ImgState::
// list_entries, the byte accounting's list size): sum over the image's blocks
// of the list length padded to whole 16-B groups, as emit_lists lays them
// out.  One workgroup per image; lengths 16 at a time ((n + 3) & ~3 per byte
// without carries: every length is <= 64), summed by v_dot4_u32_u8.
//
// The same pass takes the probe bound (bound != 0): for an
// image whose pending trial is the cached probe D.bound_node, the true list
// lengths give probe_bound(), a lower bound of that trial's file size.  Above
// the target, the trial's only possible outcome is "too big", so the search
// step decide_trial would take after coding it is taken here and k_huff /
// k_scan find the image inactive.  count: keep the padded entry count (the
// profile's byte accounting).  mins: (dcmin, acmin) for grey and for colour
// images, from the coding tables (icx_create).
__global__ __launch_bounds__(1024) void k_list_count(const ImgDesc* __restrict__ descs, ImgState* states,
                                                     const QNode* __restrict__ nodes,
                                                     const int32_t* __restrict__ ids, int m, int count, int bound,
                                                     int4 mins)
{
    __shared__ uint32_t s_w[2][16];
    const int img = ids ? ids[blockIdx.x] : (int)blockIdx.x;
    const ImgDesc& D = descs[img];
    ImgState& S = states[img];
    // workgroup-uniform: only an image the bound may decide is summed when
    // nothing is counted
    const bool try_bound = bound && D.bound_node >= 0 && S.active && !S.force && S.node == D.bound_node;
    if (!count && !try_bound) return;
    const int64_t n = D.nblocks;
    const uint8_t* nc = D.ncoef;
    const int64_t n16 = ((uintptr_t)nc & 15) ? 0 : n >> 4;
    uint32_t sum = 0, len = 0;  // padded entries; true list lengths (<= 64 per block: < 2^32 for any image)
    for (int64_t i = threadIdx.x; i < n16; i += blockDim.x) {
        const uint4 v = ld16(nc + 16 * i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sum = __builtin_amdgcn_udot4((w[k] + 0x03030303u) & 0xFCFCFCFCu, 0x01010101u, sum, false);
            len = __builtin_amdgcn_udot4(w[k], 0x01010101u, len, false);
        }
    }
    for (int64_t i = n16 * 16 + threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t v = gp(nc)[i];
        sum += (v + 3u) & ~3u;
        len += v;
    }
    sum = (uint32_t)wave_incl_scan((int)sum);
    len = (uint32_t)wave_incl_scan((int)len);
    const int lane = threadIdx.x & 63;
    if (lane == 63) {
        s_w[0][threadIdx.x >> 6] = sum;
        s_w[1][threadIdx.x >> 6] = len;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0, lens = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); i++) {
            tot += s_w[0][i];
            lens += s_w[1][i];
        }
        if (count) atomicAdd((unsigned long long*)S.list_entries, (unsigned long long)tot);
        if (try_bound) {
            const bool grey = D.ncomp == 1;
            const int64_t low = probe_bound(D.hdr_len, n, (int64_t)lens, grey ? mins.x : mins.z, grey ? mins.y : mins.w);
            if (low > D.target) {  // decide_trial's "too big" step; best_* and huff_wbytes untouched
                const QNode& N = nodes[S.node];
                if (S.ntrials <= MAX_TRIALS) {
                    S.trial_q[S.ntrials] = N.mid;
                    S.trial_size[S.ntrials] = -1;
                }
                S.ntrials++;
                S.nbounded++;
                const int next = N.child_nofit;
                S.node = next;
                S.active = next >= 0;
            }
        }
    }
}

// =================================================================== Huffman
// jcdctmgr.c: sign(c) * ((|c| + d/2) / d) for d = q<<3, via the exact float
// form of QNode (|c| <= 2^15, so y*d < 2^16 and the error stays < 2^-6/d).
__device__ __forceinline__ int quant(int c, float rcp, float bias)
{
    const int q = (int)fmaf(fabsf((float)c), rcp, bias);
    return c < 0 ? -q : q;
}

__device__ __forceinline__ int nbits(int a) { return a ? 32 - __clz(a) : 0; }

// Per-block LDS slot (odd stride: same-index words of a wave hit distinct
// banks); longer blocks spill to D.ovf.  Sized with the other k_huff LDS so a
// workgroup stays under 20 KiB (in 512 B allocation granules): 8 per CU.
#ifndef ICX_SLOT_WORDS
#define ICX_SLOT_WORDS 13
#endif
constexpr int SLOT_WORDS = ICX_SLOT_WORDS;

constexpr int SLOT_BITS = SLOT_WORDS * 32;
constexpr int AC_SIZES_ = 11;
constexpr int TAB_WORDS = 2 * 16 * AC_SIZES_ * 2 + 2 * 64 * 2 + 2 * 16;  // s_ac + s_qf + s_dc
constexpr int OUT_WORDS = 1024;  // chunk streams up to this many words are assembled in LDS
// 0xFF alignment bins of the assembled path: FF_COPIES copies per bin (lane
// mod FF_COPIES picks one), so the LDS atomics of a wave rarely collide.
constexpr int FF_COPIES = 16;
constexpr int TABLE_LDS_WORDS = TAB_WORDS > OUT_WORDS + 8 + 8 * FF_COPIES ? TAB_WORDS : OUT_WORDS + 8 + 8 * FF_COPIES;
constexpr int AC_SIZES = 11;                // AC magnitude categories 0..10 (8-bit JPEG)
constexpr int AC_ENTRIES = 16 * AC_SIZES;   // (run, size) slots per table

// Per-thread bit sinks: a 64-bit accumulator flushing whole 32-bit words.
// LdsSink writes the thread's LDS slot, clamped to its last word; a block that
// outgrows the slot (bits > SLOT_BITS) is coded again into a GlobalSink.
struct LdsSink {
    uint64_t acc;
    int n;
    uint32_t wb, wlast;  // byte offsets into `slots` of the next and the last slot word
    uint32_t* slots;
    __device__ __forceinline__ void put(uint32_t v, int len)  // len <= 32
    {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            *(uint32_t*)((char*)slots + min(wb, wlast)) = (uint32_t)(acc >> n);
            wb += 4;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (n) *(uint32_t*)((char*)slots + min(wb, wlast)) = (uint32_t)(acc << (32 - n));
    }
};


struct GlobalSink {
    uint64_t acc;
    int n, widx;
    GAS uint32_t* w;
    __device__ __forceinline__ void put(uint32_t v, int len)
    {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            w[widx++] = (uint32_t)(acc >> n);
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (n) w[widx] = (uint32_t)(acc << (32 - n));
    }
};

// Candidate-list entries of one block held in registers from the start (four
// 16-B groups); the rest is read from HBM one group ahead of its use.
#ifndef ICX_PRE
#define ICX_PRE 24  // list entries loaded up front (24: the most that keeps 64 VGPRs, 8 waves/SIMD)
#endif
constexpr int PRE = ICX_PRE;

// The prologue's list groups are loaded whether or not they hold entries of
// the block: a load under an exec mask is merged with its default by a copy,
// and the copy waits for the load at once - the group loads would run one
// after another.  Entries past the block's length (the following blocks'
// lists) are never coded (encode_block checks the index against the length).
// A block's list starts at most 64 entries before the end of its FDCT wave's
// reserved region, so every load stays inside that region.
__device__ __forceinline__ void load_group(uint32_t (&g)[4], const uint32_t* lst, int j)
{
    const uint4 v = ld16(lst + j);
    g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
}

__device__ __forceinline__ void load_list(uint32_t (&ev)[PRE], const uint32_t* lst)
{
#pragma unroll
    for (int g = 0; g < PRE / 4; g++) {
        uint32_t w[4];
        load_group(w, lst, 4 * g);
#pragma unroll
        for (int j = 0; j < 4; j++) ev[4 * g + j] = w[j];
    }
}

// encode_one_block (jchuff.c) of one 8x8 block from its candidate list
// (entries float_bits(c) | (k << 3), zig-zag order, entry 0 = DC, zero entries past the
// end): DC difference, then the AC run/size codes of the entries that
// quantise to nonzero — zero runs are index gaps, since every coefficient
// missing from the list quantises to zero at this trial's quality.  qf/ac/dc
// are the LDS tables of the block's component (ac entries: (code << size,
// len + size) at [run * AC_SIZES + size]).  The next entry's quantiser
// constants are read while the current one is coded.
// Quantiser constants of an entry's component and zig-zag index: entry &
// 0x3F8 is their byte offset in the [2][64] table (one VALU op for the LDS
// address, no per-lane table base).
__device__ __forceinline__ float2 qent(const float2* qf, uint32_t e)
{
    return *(const float2*)((const char*)qf + (e & 0x3F8u));
}

// ac[run * AC_SIZES + sz] (ac: an LDS table): the address as one
// v_mad_u32_u24 (the row stride held in a VGPR by the caller: as an SGPR
// operand it is rematerialised at every site) and one v_lshl_add_u32 - the
// compiler's own form is a multiply, a shift and an add3.
typedef const __attribute__((address_space(3))) uint64_t* lds_u64_cp;
__device__ __forceinline__ uint2 ac_entry(const uint2* ac, uint32_t run, int sz, uint32_t stride)
{
    uint32_t row;
    asm("v_mad_u32_u24 %0, %1, %2, %3"
        : "=v"(row)
        : "v"(run), "v"(stride), "v"((uint32_t)(uintptr_t)(lds_u64_cp)ac));
    const uint64_t v = *(lds_u64_cp)(uintptr_t)(row + ((uint32_t)sz << 3));
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}

template <class Sink>
__device__ __forceinline__ void encode_block(Sink& sink, const uint32_t (&ev)[PRE], const uint32_t* lst, int cnt,
                                             int diff, const float2* qf, const uint2* ac, const uint32_t* dc)
{
    {
        const int ds = nbits(diff < 0 ? -diff : diff);
        const uint32_t hc = dc[ds];
        const uint32_t mag = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << ds) - 1);
        sink.put(((hc >> 8) << ds) | mag, (int)(hc & 255) + ds);
    }
    const uint2 zrl = ac[15 * AC_SIZES];
    uint32_t stride = AC_SIZES * sizeof(uint2);  // ac_entry's row stride, once in a VGPR
    asm("" : "+v"(stride));
    uint32_t last = 0;  // zig-zag index of the last nonzero coefficient
    uint32_t g0[4] = {0u, 0u, 0u, 0u}, g1[4];
    load_group(g1, lst, PRE);
    uint32_t en = ev[1];
    float2 qn = qent(qf, en);
#pragma unroll
    for (int i = 1; i < 64; i++) {
        // every list of the wave is done (checked at every entry: the lists'
        // padding to whole 16-B groups is never coded, and the test is a
        // scalar compare against the wave's lane mask)
        if (!__any(i < cnt)) break;
        const uint32_t e = en;
        const float2 qk = qn;
        if (i + 1 < 64) {
            const int j = i + 1;
            if (j < PRE) {
                en = ev[j];
            } else {
                if ((j & 3) == 0) {
#pragma unroll
                    for (int q = 0; q < 4; q++) g0[q] = g1[q];
                    // the group after next, only while the block's list has one: a
                    // lane past its list would keep fetching the following
                    // lists' lines for as long as the wave's longest list
                    // runs (unconditional: 127 instead of 77 B fetched per
                    // block-trial, trial +2.7 %)
                    if (j + 4 < cnt) load_group(g1, lst, j + 4);
                }
                en = g0[j & 3];
            }
            qn = qent(qf, en);
        }
        const float f = __uint_as_float(e & ~0x3FFu);  // the coefficient (exact: integer, |c| < 2^14)
        // the quotient (exact for every |c| and divisor: tests/test_quant_exact.py),
        // nonzero iff y >= 1 - no threshold table: 8-B quantiser reads
        const float y = fmaf(fabsf(f), qk.x, qk.y);
        if (i < cnt && y >= 1.0f) {
            const uint32_t k = (e >> 3) & 63;
            uint32_t run = k - last - 1;
            while (run >= 16) {
                sink.put(zrl.x, (int)zrl.y);
                run -= 16;
            }
            const uint32_t u = (uint32_t)y;                    // |q| >= 1
            const int sz = __builtin_amdgcn_frexp_expf(y);     // bit length of |q|
            const uint2 c2 = ac_entry(ac, run, sz, stride);
            const uint32_t sm = (uint32_t)((int32_t)e >> 31);
            sink.put(c2.x | ((u ^ sm) & ((1u << sz) - 1)), (int)c2.y);
            last = k;
        }
    }
    if (last != 63) sink.put(ac[0].x, (int)ac[0].y);  // EOB
}

#ifndef ICX_HUFF_ZERO16
#define ICX_HUFF_ZERO16 1  // zero the assembly LDS with 16-B stores (-0.9 % huff, ab_r3zp_huff_zero16.txt)
#endif
#ifndef ICX_HUFF_WGS
#define ICX_HUFF_WGS 8  // workgroups per CU k_huff is compiled for (8: <= 64 VGPRs)
#endif

// One workgroup = one chunk of CHUNK_BLOCKS scan blocks; one thread = one
// 8x8 block (encode_one_block, jchuff.c), run once per trial:
//   1. quantise + Huffman-code the thread's block straight into its LDS slot
//      (coefficient quads read 512 B-coalesced from the interleaved layout)
//   2. workgroup scan of the block bit counts -> offsets inside the chunk
//   3. every run of eight 1-bits inside the chunk is binned by start position
//      mod 8 (chunk_ffa), by the thread of the block it starts in: the chunk's
//      0xFF-byte count for each alignment the chunk may land on once k_scan
//      places it.
//   4. gather: every 32-bit word of the chunk stream is assembled by the
//      thread whose block holds the word's first bit (reading the following
//      blocks' slots as needed) and stored once to scratch[cur].
__global__ __launch_bounds__(HUFF_THREADS, ICX_HUFF_WGS) void k_huff(const ImgDesc* __restrict__ descs,
                                                       const ImgState* __restrict__ states,
                                                       const QNode* __restrict__ nodes,
                                                       const int32_t* __restrict__ ids,
                                                       const int64_t* __restrict__ prefix, int m, int rev)
{
    __shared__ uint32_t slots[CHUNK_BLOCKS * SLOT_WORDS];
    // Coding tables during phase 1; afterwards the same LDS holds the chunk's
    // assembled stream (phase 3, chunks of at most OUT_WORDS words).
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[TABLE_LDS_WORDS];
    uint2 (*s_ac)[AC_ENTRIES] = (uint2 (*)[AC_ENTRIES])s_tab;
    float2 (*s_qf)[64] = (float2 (*)[64])(s_tab + 2 * AC_ENTRIES * 2);  // (frcp, fbias) per zig-zag index
    uint32_t (*s_dc)[16] = (uint32_t (*)[16])(s_tab + 2 * AC_ENTRIES * 2 + 2 * 64 * 2);
    uint32_t* const s_out = s_tab;
    __shared__ uint32_t s_off[CHUNK_BLOCKS + 1];
    __shared__ uint32_t s_bits[CHUNK_BLOCKS];
    __shared__ uint32_t s_wsum[CHUNK_BLOCKS / 64];

    // 2-D launch (every image of the plan has as many chunks): slot = y, in
    // reverse order on every other trial (rev), so a trial starts with the
    // images whose lists the previous one read last - still in the Infinity Cache
    const int slot = gridDim.y > 1 ? (int)(rev ? gridDim.y - 1 - blockIdx.y : blockIdx.y)
                                   : find_slot(prefix, m, blockIdx.x);
    const int img = ids ? ids[slot] : slot;
    const ImgState& S = states[img];
    const ImgDesc& D = descs[img];
    // An image with no trial pending (its search ended, or the probe bound
    // decided its probe: k_list_count) leaves on the first wait: its state's
    // flag comes in with the descriptor fields the prologue needs anyway
    // (the empty asm keeps those loads in front of the exit: sunk behind it,
    // each would be a wait of its own for the images still searching).
    const int active = S.active;
    const int64_t nblocks = D.nblocks;
    const int ncomp = D.ncomp;
    const GAS uint32_t* coff = gp(D.coff);
    const GAS uint8_t* ncoef = gp(D.ncoef);
    asm volatile("" ::"s"(nblocks), "s"(ncomp), "s"(coff), "s"(ncoef));
    if (!active) return;
    const int chunk = gridDim.y > 1 ? (int)blockIdx.x : (int)(blockIdx.x - prefix[slot]);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;

    const int64_t b0 = (int64_t)chunk * CHUNK_BLOCKS;
    const int nb = (int)min((int64_t)CHUNK_BLOCKS, nblocks - b0);
    const bool valid = t < nb;
    const int64_t b = b0 + t;
    int tb = 0;
    int64_t pb;
    if (ncomp == 3) {
        const uint32_t k6 = ((uint32_t)(chunk % 3) * 4u + (uint32_t)t) % 6u;  // b % 6, b0 = 256 chunk
        tb = k6 >= 4;
        if (k6 >= 1 && k6 <= 3) pb = b - 1;
        else if (k6 == 0) pb = b >= 6 ? b - 3 : -1;
        else pb = b >= 6 ? b - 6 : -1;
    } else {
        pb = b - 1;
    }
    // The prologue's loads go out in two rounds with one wait between them
    // (issued one after another with a wait each, they were a chain of about
    // eight memory latencies in front of every chunk): first the block's
    // list length and offset, the DC predictor's list offset and the coding
    // tables (the list meta depends only on the descriptor, so it goes out
    // before the rest of the image's state - node, buffer - is waited for);
    // then, once the tables are in LDS, the list itself and the predictor's
    // DC entry (the list groups are loaded unconditionally, see load_group).
    // The DC predictor (the previous block of the same component: 1, 3 or 6
    // blocks back) of most blocks is coded by a lane of the same wave, which
    // hands its quantised DC over by ds_bpermute - no workgroup barrier.  A
    // predecessor in another wave or in the previous chunk (a wave's first
    // lanes): its list offset and DC entry are fetched alongside this block's
    // own, and its DC quantised here.
    const bool in_wave = pb >= b0 && (int)(pb - b0) >= (t & ~63);
    const bool ext_prev = valid && pb >= 0 && !in_wave;  // (a lane past the chunk's blocks reads nothing)
    const int cnt = valid ? (int)ncoef[b] : 0;
    const uint32_t my_off = coff[valid ? b : b0];
    const uint32_t prev_off = coff[ext_prev ? pb : b0];
    const QNode& N = nodes[S.node];
    const int cur = S.cur;
    const float4 qv = N.qf[(t >> 6) & 1][t & 63];  // used by t < 128
    // AC codes pre-shifted for their (run, size) slot: (code << size, len + size)
    static_assert(2 * AC_ENTRIES <= 2 * CHUNK_BLOCKS, "two AC entries per thread");
    const uint2 ac0 = (&c_acx[0][0])[t];
    const bool has_ac1 = t + CHUNK_BLOCKS < 2 * AC_ENTRIES;
    const uint2 ac1 = (&c_acx[0][0])[has_ac1 ? t + CHUNK_BLOCKS : t];
    const uint32_t dcv = c_dc[(t >> 4) & 1][t & 15];  // used by t < 32
    if (t < 128) s_qf[t >> 6][t & 63] = make_float2(qv.y, qv.z);
    (&s_ac[0][0])[t] = ac0;
    if (has_ac1) (&s_ac[0][0])[t + CHUNK_BLOCKS] = ac1;
    if (t < 32) s_dc[t >> 4][t & 15] = dcv;
    __builtin_amdgcn_sched_barrier(0);  // the table registers die before the list arrives
    const uint32_t* lst = (const uint32_t*)D.coefs + 4 * (size_t)my_off;
    uint32_t ev[PRE];
    load_list(ev, lst);
    const int32_t prev_dc_raw = gp(D.coefs)[4 * (size_t)prev_off];
    __syncthreads();  // tables ready

    const float2 q0t = s_qf[tb][0];
    const int dq = quant((int)__uint_as_float(ev[0] & ~0x3FFu), q0t.x, q0t.y);
    const int from = __builtin_amdgcn_ds_bpermute((in_wave ? (int)(pb - b0) & 63 : lane) << 2, dq);
    int qprev = 0;
    if (in_wave) qprev = from;
    else if (ext_prev) qprev = quant((int)__uint_as_float((uint32_t)prev_dc_raw & ~0x3FFu), q0t.x, q0t.y);

    // ---- 1. encode_one_block into the slot (rarely: into the block's HBM spill)
    int bits = 0;
    if (valid) {
        const uint32_t sb = (uint32_t)(t * SLOT_WORDS * 4);
        LdsSink sink{0, 0, sb, sb + (SLOT_WORDS - 1) * 4, slots};
        encode_block(sink, ev, lst, cnt, dq - qprev, &s_qf[0][0], s_ac[tb], s_dc[tb]);
        bits = (int)(sink.wb - sb) * 8 + sink.n;
        sink.finish();
        if (bits > SLOT_BITS) {  // rare: reload the list (ev[] is dead by now)
            uint32_t e2[PRE];
            load_list(e2, lst);
            GlobalSink g{0, 0, 0, gp(D.ovf + b * BLOCK_WORDS)};
            encode_block(g, e2, lst, cnt, dq - qprev, &s_qf[0][0], s_ac[tb], s_dc[tb]);
            g.finish();
        }
    }

    // ---- 2. exclusive scan of block bits
    const int incl = wave_incl_scan(bits);
    if (lane == 63) s_wsum[wv] = incl;
    __syncthreads();
    uint32_t off = incl - bits, total = 0;
#pragma unroll
    for (int i = 0; i < CHUNK_BLOCKS / 64; i++) {
        if (i < wv) off += s_wsum[i];
        total += s_wsum[i];
    }
    s_off[t] = off;
    s_bits[t] = bits;
    // 0xFF alignment bins, [8][FF_COPIES] over the dead tables (past the
    // assembled stream): FF_COPIES copies per bin, picked by lane, so that the
    // LDS atomics of a wave rarely collide on one address
    uint32_t* const s_bin = s_tab + OUT_WORDS + 8;
    if (total > (uint32_t)OUT_WORDS * 32) {
        if (t < 8 * FF_COPIES) s_bin[t] = 0u;
    } else {  // the assembled stream and its bins start zeroed (tables are dead)
#if ICX_HUFF_ZERO16
        static_assert((OUT_WORDS + 8 + 8 * FF_COPIES) % 4 == 0, "whole 16-B groups");
        for (uint32_t i = t; i < (OUT_WORDS + 8 + 8 * FF_COPIES) / 4; i += CHUNK_BLOCKS)
            ((uint4*)s_tab)[i] = make_uint4(0u, 0u, 0u, 0u);
#else
        for (uint32_t i = t; i < OUT_WORDS + 8 + 8 * FF_COPIES; i += CHUNK_BLOCKS) s_tab[i] = 0u;
#endif
    }
    __syncthreads();

    const GAS uint32_t* spill0 = gp(D.ovf + b0 * BLOCK_WORDS);
    auto slot_word = [&](int u, uint32_t wi) -> uint32_t {  // word wi of block u's stream
        return s_bits[u] <= SLOT_BITS ? slots[u * SLOT_WORDS + wi] : spill0[(size_t)u * BLOCK_WORDS + wi];
    };
    GAS uint32_t* dst = gp(D.scratch[cur] + (size_t)chunk * CHUNK_WORDS);

    if (total <= (uint32_t)OUT_WORDS * 32) {
        // ---- 3. (common case) assemble the chunk stream in LDS over the dead
        // tables: every block ORs its words in at its offset; then each word is
        // stored once (coalesced) and the runs of eight 1-bits starting in it
        // (with the next word's first 7 bits; zeros past the chunk's last bit,
        // k_scan checks the boundary bytes) are binned by chunk-local start
        // position mod 8 (s_bin): the chunk's 0xFF-byte count for each
        // alignment k_scan may place it at.
        const uint32_t nwords = (total + 31) >> 5;
        if (bits > 0) {
            const uint32_t sh = off & 31, nwb = ((uint32_t)bits + 31) >> 5;
            uint32_t* o = s_out + (off >> 5);
            for (uint32_t i = 0; i < nwb; i++) {
                const uint32_t w = slot_word(t, i);
                atomicOr(o + i, w >> sh);
                if (sh) atomicOr(o + i + 1, w << (32 - sh));
            }
        }
        __syncthreads();
        for (uint32_t j = t; j < nwords; j += CHUNK_BLOCKS) {
            const uint32_t w = s_out[j];
            dst[j] = w;
            uint64_t x = ((uint64_t)w << 32) | s_out[j + 1];
            x &= x << 1;
            x &= x << 2;
            x &= x << 4;
            const uint32_t r = (uint32_t)(x >> 32);  // bit 31-d: a run starts at chunk bit 32j+d
            if (r) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int n = __popc(r & (0x80808080u >> k));
                    if (n) atomicAdd(&s_bin[k * FF_COPIES + (lane & (FF_COPIES - 1))], (uint32_t)n);
                }
            }
        }
        __syncthreads();  // bins complete
        if (t < 8) {
            uint32_t n = 0;
#pragma unroll
            for (int i = 0; i < FF_COPIES; i++) n += s_bin[t * FF_COPIES + i];
            D.chunk_ffa[cur][chunk * 8 + t] = n;
        }
        if (t == 0) D.chunk_bits[cur][chunk] = total;
        return;
    }

    // ---- 3. (long chunks) 0xFF candidates: every run of eight 1-bits that starts in this
    // block, binned by chunk-local start position mod 8 (s_bin) - the chunk's
    // 0xFF-byte count for each alignment k_scan may place it at.  Runs may
    // reach into the following blocks (their first <= 8 bits); nothing
    // follows the chunk's last bit here (k_scan checks the boundary bytes).
    if (bits > 0) {
        uint32_t la = 0;  // the <= 8 bits after this block, MSB-aligned
        int have = 0;
        for (int u = t + 1; have < 8 && u < nb; u++) {
            const int take = min(8 - have, (int)s_bits[u]);
            la |= (slot_word(u, 0) & ~(~0u >> take)) >> have;
            have += take;
        }
        const uint32_t nwb = ((uint32_t)bits + 31) >> 5;
        uint32_t cw = slot_word(t, 0);
        for (uint32_t i = 0; i < nwb; i++) {
            const uint32_t nx = i + 1 < nwb ? slot_word(t, i + 1) : 0u;
            uint64_t x = ((uint64_t)cw << 32) | nx;
            const int rem = bits - 32 * (int)i;  // block bits from word i on
            if (rem <= 32) x |= (uint64_t)la << (32 - rem);
            else if (rem < 40) x |= (uint64_t)(la >> (rem - 32));
            x &= x << 1;
            x &= x << 2;
            x &= x << 4;
            uint32_t r = (uint32_t)(x >> 32);  // bit 31-d: a run starts at block bit 32i+d
            if (rem < 32) r &= ~(~0u >> rem);
            if (r) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int n = __popc(r & (0x80808080u >> k));
                    if (n) atomicAdd(&s_bin[((off + k) & 7) * FF_COPIES + (lane & (FF_COPIES - 1))], (uint32_t)n);
                }
            }
            cw = nx;
        }
    }

    // ---- 4. gather the chunk's words
    for (uint32_t j = (off + 31) >> 5; j * 32 < off + bits; j++) {
        uint32_t outw = 0;
        int have = 0, u = t;
        uint32_t p = j * 32 - off;
        while (have < 32 && u < nb) {
            const int avail = (int)s_bits[u] - (int)p;
            const int take = min(32 - have, avail);
            const uint32_t wi = p >> 5, sh = p & 31;
            uint32_t v = slot_word(u, wi) << sh;
            if (sh + take > 32) v |= slot_word(u, wi + 1) >> (32 - sh);
            v &= take == 32 ? ~0u : ~(~0u >> take);
            outw |= v >> have;
            have += take;
            u++;
            p = 0;
        }
        dst[j] = outw;
    }
    __syncthreads();  // bins complete
    if (t < 8) {
        uint32_t n = 0;
#pragma unroll
        for (int i = 0; i < FF_COPIES; i++) n += s_bin[t * FF_COPIES + i];
        D.chunk_ffa[cur][chunk * 8 + t] = n;
    }
    if (t == 0) D.chunk_bits[cur][chunk] = total;
}

// 32 bits of the image's entropy stream starting at global bit gbit (inside
// chunk c): from chunk c, the next chunk, then the 1-bit padding of flush_bits.
__device__ __forceinline__ uint32_t stream_bits(const GAS uint32_t* __restrict__ scratch,
                                                const GAS uint64_t* __restrict__ off, int nchunks, int c,
                                                uint64_t gbit)
{
    const uint64_t start = off[c], end = off[c + 1];
    const GAS uint32_t* cs = scratch + (size_t)c * CHUNK_WORDS;
    const uint64_t s = gbit - start;
    const uint32_t lw = (uint32_t)(s >> 5), sh = (uint32_t)(s & 31);
    uint32_t v = cs[lw] << sh;
    if (sh) v |= cs[lw + 1] >> (32 - sh);
    uint64_t avail = end - gbit;
    if (avail >= 32) return v;
    v &= ~0u << (32 - avail);
    int have = (int)avail;
    if (c + 1 < nchunks) {
        const uint64_t nlen = off[c + 2] - end;
        const GAS uint32_t* ns = scratch + (size_t)(c + 1) * CHUNK_WORDS;
        uint32_t nv = ns[0];
        int take = (int)min((uint64_t)(32 - have), nlen);
        if (take > 0) {
            uint32_t piece = nv & (take == 32 ? ~0u : ~0u << (32 - take));
            v |= piece >> have;
            have += take;
        }
        // Every chunk but the last holds >= CHUNK_BLOCKS * 4 bits, so a word
        // left short here ends in the last chunk: the rest is padding.
    }
    if (have < 32) v |= ~0u >> have;  // flush_bits: pad with 1-bits
    return v;
}

// Exact file size of the pending trial, then one step of
// findBestQualityByBinarySearch (ImageCompressionJpg.java:176-189); run by
// thread 0 of the image's k_scan workgroup once the trial's totals are known.
__device__ __forceinline__ void decide_trial(const ImgDesc& D, ImgState& S, const QNode* __restrict__ nodes,
                                             uint64_t total_bits, uint32_t ff_total)
{
    const int cur = S.cur;
    S.total_bits[cur] = total_bits;
    S.ff_total[cur] = ff_total;
    S.huff_wbytes += (total_bits + 7) / 8 + (uint64_t)D.nchunks * 36;
    const int64_t size = (int64_t)D.hdr_len + (int64_t)((total_bits + 7) >> 3) + (int64_t)ff_total + 2;
    const QNode& N = nodes[S.node];
    if (S.ntrials <= MAX_TRIALS) {
        S.trial_q[S.ntrials] = N.mid;
        S.trial_size[S.ntrials] = size;
    }
    S.ntrials++;
    const bool fits = S.force || size <= D.target;  // currentSize <= targetMaxSizeBytes
    int next;
    if (fits) {
        S.best_node = S.node;
        S.best_buf = cur;
        S.best_size = size;
        S.cur = cur ^ 1;
        next = N.child_fit;
    } else {
        next = N.child_nofit;
    }
    if (S.force) next = -1;
    S.node = next;
    S.active = next >= 0;
}

// Exclusive scan of `n` per-chunk counts by one 1024-thread workgroup: every
// thread sums a run of consecutive chunks (one pass whatever n is: an 8K frame
// has ~3000 chunks), a 64-bit wave scan and the wave totals place the
// runs, then every thread writes its run's offsets.  Returns the total to
// every thread.
template <class Get, class Put>
__device__ __forceinline__ uint64_t wg_exclusive_scan(int n, Get get, Put put, uint64_t (&s_w)[16])
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (n + 1023) >> 10;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    uint64_t sum = 0;
    for (int i = i0; i < i1; i++) sum += get(i);
    uint64_t x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint64_t base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (k < wv) base += s_w[k];
        total += s_w[k];
    }
    base += x - sum;
    for (int i = i0; i < i1; i++) {
        const uint64_t v = get(i);
        put(i, base);
        base += v;
    }
    return total;
}

// One workgroup per image: exclusive scan of the chunk bit counts, then each
// chunk's 0xFF count: its alignment bin chunk_ffa[(8 - off%8) % 8] plus the
// byte that starts in the chunk and ends in the next one (or in the padding).
__global__ __launch_bounds__(1024) void k_scan(const ImgDesc* __restrict__ descs, ImgState* states,
                                               const QNode* __restrict__ nodes, const int32_t* __restrict__ ids,
                                               int m)
{
    __shared__ uint64_t s_w[16];
    const int img = ids ? ids[blockIdx.x] : (int)blockIdx.x;
    ImgState& S = states[img];
    if (!S.active) return;
    const ImgDesc& D = descs[img];
    const int cur = S.cur;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const GAS uint32_t* bits = gp(D.chunk_bits[cur]);
    GAS uint64_t* offw = gp(D.chunk_off[cur]);
    const uint64_t total = wg_exclusive_scan(
        D.nchunks, [&](int i) -> uint64_t { return bits[i]; }, [&](int i, uint64_t o) { offw[i] = o; }, s_w);
    if (t == 0) offw[D.nchunks] = total;
    __syncthreads();
    const GAS uint64_t* off = gp(D.chunk_off[cur]);
    const GAS uint32_t* ffa = gp(D.chunk_ffa[cur]);
    uint32_t sum = 0;
    for (int i = t; i < D.nchunks; i += 1024) {
        const uint64_t o = off[i], e = off[i + 1];
        uint32_t n = ffa[i * 8 + ((8 - (o & 7)) & 7)];
        if ((e & 7) && (e & ~(uint64_t)7) >= o &&
            (stream_bits(gp(D.scratch[cur]), off, D.nchunks, i, e & ~(uint64_t)7) >> 24) == 0xFF)
            n++;
        D.chunk_ff[cur][i] = n;
        sum += n;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    __syncthreads();
    if (lane == 0) s_w[wv] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t ff = 0;
        for (int k = 0; k < 16; k++) ff += s_w[k];
        decide_trial(D, S, nodes, total, (uint32_t)ff);
    }
}

// Final pass 1 (one workgroup per image): exclusive scan of the best trial's
// per-chunk 0xFF counts -> stuffed byte offsets; file length and capacity check.
__global__ __launch_bounds__(1024) void k_ffscan(const ImgDesc* __restrict__ descs, ImgState* states,
                                                 const int32_t* __restrict__ ids, int m)
{
    __shared__ uint64_t s_w[16];
    const int img = ids ? ids[blockIdx.x] : (int)blockIdx.x;
    ImgState& S = states[img];
    if (S.best_node < 0) return;
    const ImgDesc& D = descs[img];
    const int buf = S.best_buf;
    const GAS uint32_t* ff = gp(D.chunk_ff[buf]);
    GAS uint64_t* ffoff = gp(D.chunk_ffoff);
    const uint64_t total = wg_exclusive_scan(
        D.nchunks, [&](int i) -> uint64_t { return ff[i]; }, [&](int i, uint64_t o) { ffoff[i] = o; }, s_w);
    if (threadIdx.x == 0) {
        const uint64_t nbytes = (D.chunk_off[buf][D.nchunks] + 7) >> 3;
        const int64_t len = (int64_t)D.hdr_len + (int64_t)nbytes + (int64_t)total + 2;
        S.out_len = len;
        S.status = (uint64_t)len > D.cap ? 4 : 0;
    }
}

// Final pass 2 (one wave per chunk): header (chunk 0), stuffed entropy bytes
// of the bytes the chunk owns (first bit inside it), EOI (last chunk), written
// straight into the caller's output buffer: 256 source bytes per step are
// stuffed into the wave's LDS stage and leave as aligned dwords.
#ifndef ICX_STUFF_BATCH
#define ICX_STUFF_BATCH 3  // measured: 3 beats 2, 4, 6, 8, 16 (fewer VGPRs, more waves in flight)
#endif
constexpr int STUFF_BATCH = ICX_STUFF_BATCH;  // 256-byte pieces whose source loads k_stuff issues together

__global__ __launch_bounds__(256) void k_stuff(const ImgDesc* __restrict__ descs, const ImgState* __restrict__ states,
                                               const QNode* __restrict__ nodes, const int32_t* __restrict__ ids,
                                               const int64_t* __restrict__ prefix, int m)
{
    __shared__ uint32_t s_stg[4][132];  // per wave: one stuffed piece (<= 512 B) + read-ahead
    // wave-uniform (readfirstlane: the chunk's state and descriptor fields then
    // come in scalar loads)
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int slot, c;
    if (gridDim.y > 1) {  // 2-D launch: slot = y, every image has gridDim.x * 4 >= nchunks
        slot = (int)blockIdx.y;
        c = (int)item;
    } else {
        if (item >= prefix[m]) return;
        slot = find_slot(prefix, m, item);
        c = (int)(item - prefix[slot]);
    }
    const int img = ids ? ids[slot] : slot;
    const ImgState& S = states[img];
    const ImgDesc& D = descs[img];
    // The prologue's loads in three rounds (state and descriptor fields; the
    // chunk's offsets; its stream words), each issued whole before the early
    // exits - one after another, with the exits between them, they were a
    // chain of about ten memory latencies in front of a chunk's few hundred
    // bytes of work.  Indices are clamped so every load is in bounds.
    const int best = S.best_node, status = S.status, buf = S.best_buf & 1, nch = D.nchunks;
    const GAS uint64_t* off = gp(buf ? D.chunk_off[1] : D.chunk_off[0]);
    const int cc = min(c, nch - 1);
    const uint64_t total = off[nch], start = off[cc], end = off[cc + 1];
    uint64_t run = gp(D.chunk_ffoff)[cc];
    if (best < 0 || status != 0 || c >= nch) return;
    const int lane = threadIdx.x & 63;
    GAS uint8_t* out = gp(D.out);
    const uint64_t nbytes = (total + 7) >> 3;
    const int hdr = D.hdr_len;

    if (c == 0) {  // marker segments: template + DQT payload + SOF dimensions
        const QNode& N = nodes[S.best_node];
        const bool colour = D.ncomp == 3, grouped = hdr == HDR_COLOR_GROUPED || hdr == HDR_GRAY_GROUPED;
        const uint8_t* tpl = c_hdr[2 * grouped + colour];
        const int q1 = hdr_dqt1(grouped), sof = hdr_sof(colour, grouped);
        for (int i = lane; i < hdr; i += 64) {
            uint8_t v = tpl[i];
            if (i >= 25 && i < 89) v = (uint8_t)N.qt[0][c_zz_to_nat[i - 25]];
            else if (colour && i >= q1 && i < q1 + 64) v = (uint8_t)N.qt[1][c_zz_to_nat[i - q1]];
            if (i == sof + 5) v = (uint8_t)(D.h >> 8);
            if (i == sof + 6) v = (uint8_t)D.h;
            if (i == sof + 7) v = (uint8_t)(D.w >> 8);
            if (i == sof + 8) v = (uint8_t)D.w;
            out[i] = v;
        }
    }
    const uint64_t bb = (start + 7) >> 3;                  // owned bytes [bb, be)
    const uint64_t be = min((end + 7) >> 3, nbytes);
    const GAS uint32_t* cs = gp(buf ? D.scratch[1] : D.scratch[0]) + (size_t)c * CHUNK_WORDS;
    uint32_t* stw = s_stg[threadIdx.x >> 6];                 // this wave's stage
    uint8_t* stb = (uint8_t*)stw;
    for (uint64_t qb = bb; qb < be; qb += 256 * STUFF_BATCH) {
        // 0. the source words of up to STUFF_BATCH pieces, all loads in flight
        //    at once (one latency per batch, not per piece)
        uint32_t w0[STUFF_BATCH], w1[STUFF_BATCH];
#pragma unroll
        for (int it = 0; it < STUFF_BATCH; it++) {  // unconditional (clamped): see load_group
            const uint64_t q = min(qb + 256 * it + 4 * lane, be);
            const uint32_t lw = min((uint32_t)((q * 8 - start) >> 5), (uint32_t)CHUNK_WORDS - 1);
            w0[it] = cs[lw];
            w1[it] = cs[min(lw + 1, (uint32_t)CHUNK_WORDS - 1)];
        }
#pragma unroll
        for (int it = 0; it < STUFF_BATCH; it++) {
            const uint64_t q0 = qb + 256 * it;
            if (q0 >= be) break;  // wave-uniform
            // 1. four source bytes per lane, each 0xFF followed by a stuffed
            //    0x00, laid out back to back in the wave's LDS stage
            const uint64_t q = q0 + 4 * lane;                // this lane: bytes q..q+3
            const int nv = q < be ? (int)min((uint64_t)4, be - q) : 0;
            uint32_t v = 0;
            int nout = nv;
            if (nv) {
                const uint32_t sh = (uint32_t)((q * 8 - start) & 31);
                v = sh ? __builtin_amdgcn_alignbit(w0[it], w1[it], 32 - sh) : w0[it];
                if (end - q * 8 < 32)  // the chunk's last bits: next chunk / padding
                    v = stream_bits(gp(D.scratch[buf]), off, D.nchunks, c, q * 8);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < nv && ((v >> (24 - 8 * j)) & 255) == 255) nout++;
            }
            const int incl = wave_incl_scan(nout);
            const int len = __builtin_amdgcn_readlane(incl, 63);  // stuffed bytes of this piece
            int p = incl - nout;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j < nv) {
                    const uint8_t byte = (uint8_t)(v >> (24 - 8 * j));
                    stb[p++] = byte;
                    if (byte == 0xFF) stb[p++] = 0;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // 2. the piece leaves as aligned dword stores plus at most 3 + 3
            //    byte stores at its ends (neighbouring chunks own the bytes around it)
            const uint64_t g = (uint64_t)hdr + q0 + run;     // output offset of the piece
            const int head = min((int)((4 - (((uintptr_t)D.out + g) & 3)) & 3), len);  // to a 4-B boundary
            const int nd = (len - head) >> 2, tail = len - head - 4 * nd;
            if (lane < head) out[g + lane] = stb[lane];
            if (lane < tail) out[g + head + 4 * nd + lane] = stb[head + 4 * nd + lane];
            GAS uint32_t* od = (GAS uint32_t*)(out + g + head);
            for (int i = lane; i < nd; i += 64) {
                const int s = head + 4 * i;
                od[i] = __builtin_amdgcn_alignbyte(stw[(s >> 2) + 1], stw[s >> 2], (uint32_t)(s & 3));
            }
            __builtin_amdgcn_wave_barrier();
            run += (uint64_t)(len - (int)min((uint64_t)256, be - q0));  // stuffed zeros so far
        }
    }
    if (c == D.nchunks - 1 && lane == 0) {
        out[S.out_len - 2] = 0xFF;
        out[S.out_len - 1] = 0xD9;
    }
}

// =================================================================== resize
// ImageTools.resizeImage -> Graphics2D.drawImage(BILINEAR) -> Java2D
// TransformHelper: inverse scale in 32.32 fixed point, source sample at the
// pixel centre minus 0.5, edges clamped, 8-bit fraction weights, rounding at
// bit 16 (BilinearInterp).
//
// One workgroup = a tile of 64 x 16 destination pixels (4 per thread, one
// wave per destination row).  The source rectangle the tile's taps touch
// (monotone in x and y, so the taps of its corner pixels bound it) is staged
// in LDS first, by 16-B loads of whole rows - coalesced, each source byte
// fetched once per tile however many taps read it - and the taps are then
// LDS reads.  A tile whose rectangle does not fit (scales below ~0.2, where
// the taps skip most of the source anyway) reads its taps from global memory
// instead.  Several images share one launch (icx_png_fit_batch): a 2-D grid
// (x = tile, y = image) when they have as many tiles, else a slot search.
//
// Pixel classes: BPP 1 (grey), 3 (BGR / RGB: channel order does not
// matter), 2 (TYPE_USHORT_GRAY: Java2D's UshortGray loops fetch gray >> 8
// into IntArgbPre, interpolate in 8 bits and store ComposeUshortGrayFrom3-
// ByteRgb(g, g, g) = (19672 + 38621 + 7500) g >> 8 = 257 g), 4 (four-byte
// rasters, below).
constexpr int RS_TW = 64, RS_TH = 16;  // destination tile
constexpr int RS_LDS = 24576;          // source rectangle staging: 6 workgroups per CU

__device__ __forceinline__ int bilerp(int p00, int p01, int p10, int p11, int xf, int yf)
{
    const int top = (p00 << 8) + (p01 - p00) * xf;
    const int bot = (p10 << 8) + (p11 - p10) * xf;
    return ((top << 8) + (bot - top) * yf + (1 << 15)) >> 16;
}

// Four-byte pixels (ImageTools.java:12-15 keeps the source type): Java2D's
// TransformHelper fetches the four neighbours as IntArgbPre (colours times
// alpha through AlphaMath's mul8table; an opaque type's alpha is 0xff),
// interpolates the four channels, and the SrcOver mask blit onto the new
// all-zero image stores alpha 0 as a zero pixel, alpha 0xff as is, else
// un-premultiplies through div8table.  XRGB (TYPE_INT_RGB) stores 0 in its
// unused byte.  AB = alpha byte (0: ABGR, 3: BGRA / RGBA).
__device__ __forceinline__ uint32_t mul8(uint32_t a, uint32_t c)  // AlphaMath.c mul8table[a][c]
{
    return ((c * (a * 0x010101u) + (1u << 23)) >> 24) & 0xffu;
}

// the four taps fetched as IntArgbPre and interpolated: v[b] per byte b
template <int AB, bool OPAQUE>
__device__ __forceinline__ void bilerp4_pre(const uint32_t (&p)[4], int xf, int yf, int (&v)[4])
{
    uint32_t pre[4][4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t al = OPAQUE ? 255u : (p[s] >> (8 * AB)) & 255u;
#pragma unroll
        for (int b = 0; b < 4; b++) pre[s][b] = b == AB ? al : mul8(al, (p[s] >> (8 * b)) & 255u);
    }
#pragma unroll
    for (int b = 0; b < 4; b++) v[b] = bilerp(pre[0][b], pre[1][b], pre[2][b], pre[3][b], xf, yf);
}

template <int AB, bool OPAQUE>
__device__ __forceinline__ uint32_t bilerp4(const uint32_t (&p)[4], int xf, int yf)
{
    int v[4];
    bilerp4_pre<AB, OPAQUE>(p, xf, yf, v);
    const uint32_t al = (uint32_t)v[AB];
    uint32_t out = 0;
    if (OPAQUE) {
#pragma unroll
        for (int b = 0; b < 4; b++) out |= b == AB ? 0u : (uint32_t)v[b] << (8 * b);
    } else if (al == 255u) {
#pragma unroll
        for (int b = 0; b < 4; b++) out |= (uint32_t)v[b] << (8 * b);
    } else if (al != 0u) {  // div8table[al][c]: c >= al gives 255
        const uint32_t inc = ((0xffu << 24) + al / 2) / al;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t c = (uint32_t)v[b];
            const uint32_t d = b == AB ? al : c >= al ? 255u : ((1u << 23) + c * inc) >> 24;
            out |= d << (8 * b);
        }
    }
    return out;
}

// The four taps of destination pixel (dx, dy): rows ya, yb, columns xa, xb,
// 8-bit fractions xf, yf.
struct Taps {
    int ya, yb, xa, xb, xf, yf;
};
__device__ __forceinline__ void tap_x(const ResizeArgs& a, int dx, int& xa, int& xb, int& xf)
{
    const int64_t xl = a.x0l + (int64_t)dx * a.dxl - ((int64_t)1 << 31);
    const int xw = (int)(xl >> 32);
    xf = (int)((uint32_t)xl >> 24);
    if (xw < 0) xa = xb = 0; else if (xw + 1 >= a.sw) xa = xb = xw; else { xa = xw; xb = xw + 1; }
}
__device__ __forceinline__ void tap_y(const ResizeArgs& a, int dy, int& ya, int& yb, int& yf)
{
    const int64_t yl = a.y0l + (int64_t)dy * a.dyl - ((int64_t)1 << 31);
    const int yw = (int)(yl >> 32);
    yf = (int)((uint32_t)yl >> 24);
    if (yw < 0) ya = yb = 0; else if (yw + 1 >= a.sh) ya = yb = yw; else { ya = yw; yb = yw + 1; }
}

// A source sample of type T at byte address p: LDS (L) or global memory.
#define LAS __attribute__((address_space(3)))
template <class T, bool L>
__device__ __forceinline__ uint32_t ldx(const uint8_t* p)
{
    if constexpr (L) return *(const LAS T*)p;
    else return *(const GAS T*)p;
}

// Palette rasters (IDX 1: TYPE_BYTE_INDEXED, 2: TYPE_BYTE_BINARY; the source
// holds one colour-map index per byte): the taps are fetched through the
// source's map as IntArgbPre (CopyByteIndexedToIntArgbPre: mul8 premultiply)
// and interpolated as the four-byte formats are; the alpha mask blit
// (SrcOver) onto the new image - its pixel 0, opaque black in both default
// maps - leaves the premultiplied colour at alpha 255; the store picks the
// destination index through the inverse colour map (32x32x32 cells), after
// the 8x8 ordered dither errors at (x & 7, y & 7) for ByteIndexed (skipped
// when r, g, b are each 0 or 255 and the map represents the primaries; the
// components clamped to 0..255).  ByteBinary stores have no dither.
__constant__ int8_t c_dith[3][64];  // make_dither_arrays: red, green, blue errors [(y & 7) * 8 + (x & 7)]

template <int IDX>
__device__ __forceinline__ uint8_t store_indexed(const ResizeArgs& a, const int (&v)[4], int dx, int dy)
{
    int r = v[2], g = v[1], b = v[0];  // bytes B, G, R, A of 0xAARRGGBB
    if (IDX == 1) {
        const bool prim = a.prims && (r == 0 || r == 255) && (g == 0 || g == 255) && (b == 0 || b == 255);
        if (!prim) {
            const int e = ((dy & 7) << 3) | (dx & 7);
            r += c_dith[0][e];
            g += c_dith[1][e];
            b += c_dith[2][e];
        }
        r = min(max(r, 0), 255);
        g = min(max(g, 0), 255);
        b = min(max(b, 0), 255);
    }
    return gp(a.inv)[((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)];
}

// One destination pixel from the rows ra / rb (addresses of source pixel 0
// of rows ya / yb: global memory, or LDS rebased so that the same x indexes
// it), stored at o.
template <int BPP, int AB, bool OPQ, bool L, int IDX = 0>
__device__ __forceinline__ void resize_px(const uint8_t* ra, const uint8_t* rb, int xa, int xb, int xf, int yf,
                                          uint8_t* o, const ResizeArgs& a, int dx, int dy)
{
    if constexpr (IDX != 0) {
        const GAS uint32_t* pal = gp(a.pal);
        const uint32_t p[4] = {pal[ldx<uint8_t, L>(ra + xa)], pal[ldx<uint8_t, L>(ra + xb)],
                               pal[ldx<uint8_t, L>(rb + xa)], pal[ldx<uint8_t, L>(rb + xb)]};
        int v[4];
        bilerp4_pre<3, false>(p, xf, yf, v);
        *(GAS uint8_t*)o = store_indexed<IDX>(a, v, dx, dy);
    } else if constexpr (BPP == 4) {
        const uint32_t p[4] = {ldx<uint32_t, L>(ra + 4 * xa), ldx<uint32_t, L>(ra + 4 * xb),
                               ldx<uint32_t, L>(rb + 4 * xa), ldx<uint32_t, L>(rb + 4 * xb)};
        *(GAS uint32_t*)o = bilerp4<AB, OPQ>(p, xf, yf);
    } else if constexpr (BPP == 2) {
        const int v = bilerp(ldx<uint16_t, L>(ra + 2 * xa) >> 8, ldx<uint16_t, L>(ra + 2 * xb) >> 8,
                             ldx<uint16_t, L>(rb + 2 * xa) >> 8, ldx<uint16_t, L>(rb + 2 * xb) >> 8, xf, yf);
        *(GAS uint16_t*)o = (uint16_t)(v * 257);
    } else {
#pragma unroll
        for (int c = 0; c < BPP; c++)
            ((GAS uint8_t*)o)[c] = (uint8_t)bilerp(ldx<uint8_t, L>(ra + BPP * xa + c), ldx<uint8_t, L>(ra + BPP * xb + c),
                                                   ldx<uint8_t, L>(rb + BPP * xa + c), ldx<uint8_t, L>(rb + BPP * xb + c),
                                                   xf, yf);
    }
}

template <int BPP, int AB, bool OPQ, int IDX = 0>
__global__ __launch_bounds__(256) void k_resize(ResizeArgs one, const ResizeArgs* __restrict__ descs,
                                                const int64_t* __restrict__ prefix, int m)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[RS_LDS];
    int64_t tile;
    ResizeArgs a;
    if (descs) {
        const int slot = gridDim.y > 1 ? (int)blockIdx.y : find_slot(prefix, m, blockIdx.x);
        a = descs[slot];
        tile = gridDim.y > 1 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - prefix[slot];
    } else {
        a = one;
        tile = blockIdx.x;
    }
    const int ty = (int)(tile / a.tiles_x), tx = (int)(tile - (int64_t)ty * a.tiles_x);
    const int dx0 = tx * RS_TW, dy0 = ty * RS_TH;
    const int dxe = min(dx0 + RS_TW, a.dw) - 1, dye = min(dy0 + RS_TH, a.dh) - 1;
    if (dy0 >= a.dh) return;
    // the tile's source rectangle: columns bx0..bx1, rows by0..by1 (wave-uniform)
    int bx0, bx1, by0, by1, u0, u1;
    tap_x(a, dx0, bx0, u0, u1);
    tap_x(a, dxe, u0, bx1, u1);
    tap_y(a, dy0, by0, u0, u1);
    tap_y(a, dye, u0, by1, u1);
    const int n16 = (((bx1 - bx0 + 1) * BPP + 15) >> 4) + 1;  // 16-B pieces per staged row (any alignment)
    const int nrows = by1 - by0 + 1;
    const bool staged = n16 <= 64 && nrows * n16 * 16 <= RS_LDS;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int dx = dx0 + lane;
    int xa, xb, xf;
    tap_x(a, min(dx, a.dw - 1), xa, xb, xf);
    if (staged) {
        const int lstr = n16 * 16;
        // rows per wave pass: lanes split into 64 / n16p groups of n16p (power of two >= n16)
        const int n16p = n16 <= 1 ? 1 : 1 << (32 - __clz(n16 - 1));
        const int rpp = 64 / n16p, sub = lane / n16p, k = lane & (n16p - 1);
        for (int r0 = wave * rpp; r0 < nrows; r0 += 4 * rpp) {
            const int r = r0 + sub;
            if (r < nrows && k < n16) {
                const uint8_t* row = a.src + (size_t)(by0 + r) * a.sstride;
                const uintptr_t s0 = (uintptr_t)(row + (size_t)bx0 * BPP) & ~(uintptr_t)15;
                const uintptr_t e = ((uintptr_t)(row + (size_t)(bx1 + 1) * BPP) + 15) & ~(uintptr_t)15;
                // whole 16-B granules holding the row's bytes: never past the page the bytes are on
                if (s0 + 16 * (uintptr_t)k < e) *(uint4*)&lds[r * lstr + 16 * k] = ld16((const void*)(s0 + 16 * k));
            }
        }
        __syncthreads();
        if (dx > dxe) return;
#pragma unroll
        for (int q = 0; q < RS_TH / 4; q++) {
            const int dy = dy0 + wave + 4 * q;
            if (dy > dye) break;
            int ya, yb, yf;
            tap_y(a, dy, ya, yb, yf);
            // LDS row of source row y, rebased to its pixel 0: offset of pixel bx0 in its granule
            auto lrow = [&](int y) -> const uint8_t* {
                const uint32_t mis = ((uint32_t)(uintptr_t)a.src + (uint32_t)y * (uint32_t)a.sstride +
                                      (uint32_t)(bx0 * BPP)) & 15u;
                return &lds[(y - by0) * lstr + mis] - (ptrdiff_t)bx0 * BPP;
            };
            resize_px<BPP, AB, OPQ, true, IDX>(lrow(ya), lrow(yb), xa, xb, xf, yf,
                                               a.dst + (size_t)dy * a.dstride + (size_t)dx * BPP, a, dx, dy);
        }
    } else {
        if (dx > dxe) return;
        for (int q = 0; q < RS_TH / 4; q++) {
            const int dy = dy0 + wave + 4 * q;
            if (dy > dye) break;
            int ya, yb, yf;
            tap_y(a, dy, ya, yb, yf);
            resize_px<BPP, AB, OPQ, false, IDX>(a.src + (size_t)ya * a.sstride, a.src + (size_t)yb * a.sstride, xa,
                                                xb, xf, yf, a.dst + (size_t)dy * a.dstride + (size_t)dx * BPP, a,
                                                dx, dy);
        }
    }
}

// =================================================================== host side
// FNV-1a over the constant tables' bytes, in upload order (dith, nat_to_zz,
// zz_to_nat, dc, ac, acx, hdr): the device computes it from its own symbols
// (k_const_digest, one thread, ~6 KB), the host from the tables it uploads;
// icx_create compares the two on every new context (icx_runtime.cpp).
struct FnvAcc {
    uint64_t h = 0xcbf29ce484222325ull;
    __host__ __device__ void add(const void* p, int n)
    {
        const uint8_t* b = (const uint8_t*)p;
        for (int i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    }
};

__global__ void k_const_digest(uint64_t* out)
{
    if (threadIdx.x != 0) return;
    FnvAcc f;
    f.add(c_dith, sizeof(c_dith));
    f.add(c_nat_to_zz, sizeof(c_nat_to_zz));
    f.add(c_zz_to_nat, sizeof(c_zz_to_nat));
    f.add(c_dc, sizeof(c_dc));
    f.add(c_ac, sizeof(c_ac));
    f.add(c_acx, sizeof(c_acx));
    f.add(c_hdr, sizeof(c_hdr));
    *out = f.h;
}

void launch_const_digest(uint64_t* out, hipStream_t st)
{
    hipLaunchKernelGGL(k_const_digest, dim3(1), dim3(64), 0, st, out);
}

static void derive_acx(const uint32_t ac[2][256], uint2 (&acx)[2][16 * 11])
{
    for (int c = 0; c < 2; c++)
        for (int run = 0; run < 16; run++)
            for (int sz = 0; sz < 11; sz++) {
                const uint32_t h = ac[c][(run << 4) | sz];
                acx[c][run * 11 + sz] = make_uint2((h >> 8) << sz, (h & 255) + sz);
            }
}

uint64_t const_digest_host(const uint8_t nat_to_zz[64], const uint8_t zz_to_nat[64], const uint32_t dc[2][16],
                           const uint32_t ac[2][256], const uint8_t hdr[4][HDR_COLOR], const int8_t dith[3][64])
{
    uint2 acx[2][16 * 11];
    derive_acx(ac, acx);
    FnvAcc f;
    f.add(dith, 3 * 64);
    f.add(nat_to_zz, 64);
    f.add(zz_to_nat, 64);
    f.add(dc, sizeof(uint32_t) * 2 * 16);
    f.add(ac, sizeof(uint32_t) * 2 * 256);
    f.add(acx, sizeof(acx));
    f.add(hdr, 4 * HDR_COLOR);
    return f.h;
}

hipError_t upload_constants(const uint8_t nat_to_zz[64], const uint8_t zz_to_nat[64],
                            const uint32_t dc[2][16], const uint32_t ac[2][256],
                            const uint8_t hdr[4][HDR_COLOR], const int8_t dith[3][64])
{
    hipError_t e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_dith), dith, 3 * 64))) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_nat_to_zz), nat_to_zz, 64))) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_zz_to_nat), zz_to_nat, 64))) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_dc), dc, sizeof(uint32_t) * 2 * 16))) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_ac), ac, sizeof(uint32_t) * 2 * 256))) return e;
    uint2 acx[2][16 * 11];
    derive_acx(ac, acx);
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_acx), acx, sizeof(acx)))) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(c_hdr), hdr, 4 * HDR_COLOR);
}

thread_local LaunchTiming g_launch_timing;

// hipLaunchKernelGGL, or - when a Timed region handed over events - the
// extended launch that records them at the dispatch's start and end.
#define ICX_LAUNCH(K, GRID, BLOCK, SHM, ST, ...)                                                          \
    do {                                                                                                  \
        LaunchTiming& lt_ = g_launch_timing;                                                              \
        if (lt_.a) {                                                                                      \
            hipExtLaunchKernelGGL(K, GRID, BLOCK, SHM, ST, lt_.a, lt_.b, 0, __VA_ARGS__);                 \
            lt_.a = lt_.b = nullptr;                                                                      \
            lt_.used = true;                                                                              \
        } else {                                                                                          \
            hipLaunchKernelGGL(K, GRID, BLOCK, SHM, ST, __VA_ARGS__);                                     \
        }                                                                                                 \
    } while (0)

static inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// A plan over images 0..m-1 in order passes no id table: the kernels take
// slot = image and skip one dependent load at workgroup start.
static inline const int32_t* plan_ids(const Plan& p) { return p.identity ? nullptr : p.ids; }

void launch_fdct(const ImgDesc* d, ImgState* s, const QNode* n, const Plan& p, int64_t tiles, int kind,
                 hipStream_t st)
{
    if (tiles <= 0) return;
    const dim3 grid = p.uniform > 0 && p.m > 1 ? dim3(grid_of(p.uniform, FDCT_TILES), (unsigned)p.m)
                                               : dim3(grid_of(tiles, FDCT_TILES));
    if (kind == 2)
        ICX_LAUNCH(k_fdct_gray, p.uniform > 0 && p.m > 1 ? dim3((unsigned)p.uniform, (unsigned)p.m) : dim3((unsigned)tiles),
                   dim3(256), 0, st, d, n, s, plan_ids(p), p.prefix, p.m);
    else if (kind == 0)
        ICX_LAUNCH(k_fdct_color<true>, grid, dim3(256), 0, st, d, n, s, plan_ids(p), p.prefix, p.m);
    else
        ICX_LAUNCH(k_fdct_color<false>, grid, dim3(256), 0, st, d, n, s, plan_ids(p), p.prefix, p.m);
}

void launch_list_count(const ImgDesc* d, ImgState* s, const QNode* n, const Plan& p, bool count, bool bound,
                       const int32_t mins[4], hipStream_t st)
{
    ICX_LAUNCH(k_list_count, dim3(p.m), dim3(1024), 0, st, d, s, n, plan_ids(p), p.m, count ? 1 : 0, bound ? 1 : 0,
               make_int4(mins[0], mins[1], mins[2], mins[3]));
}

void launch_huff(const ImgDesc* d, const ImgState* s, const QNode* n, const Plan& p, int64_t wgs, bool rev,
                 hipStream_t st)
{
    if (wgs <= 0) return;
    const dim3 grid = p.uniform > 0 && p.m > 1 ? dim3((unsigned)p.uniform, (unsigned)p.m) : dim3((unsigned)wgs);
    ICX_LAUNCH(k_huff, grid, dim3(HUFF_THREADS), 0, st, d, s, n, plan_ids(p), p.prefix, p.m, rev ? 1 : 0);
}

void launch_scan(const ImgDesc* d, ImgState* s, const QNode* n, const Plan& p, hipStream_t st)
{
    ICX_LAUNCH(k_scan, dim3(p.m), dim3(1024), 0, st, d, s, n, plan_ids(p), p.m);
}

void launch_ffscan(const ImgDesc* d, ImgState* s, const Plan& p, hipStream_t st)
{
    ICX_LAUNCH(k_ffscan, dim3(p.m), dim3(1024), 0, st, d, s, plan_ids(p), p.m);
}

void launch_stuff(const ImgDesc* d, const ImgState* s, const QNode* n, const Plan& p, int64_t chunks, hipStream_t st)
{
    if (chunks <= 0) return;
    const dim3 grid = p.uniform > 0 && p.m > 1 ? dim3((unsigned)grid_of(p.uniform, 4), (unsigned)p.m)
                                               : dim3((unsigned)grid_of(chunks, 4));
    ICX_LAUNCH(k_stuff, grid, dim3(256), 0, st, d, s, n, plan_ids(p), p.prefix, p.m);
}

// AffineTransform.scale(dw/sw, dh/sh).createInverse(): m00 = 1.0 / (dw/sw);
// the first pixel centre (0.5) maps to 0.5 * m00.
ResizeArgs resize_args(const uint8_t* src, int sw, int sh, int sstride, int fmt, uint8_t* dst, int dw, int dh,
                       int dstride)
{
    ResizeArgs a;
    a.src = src; a.dst = dst;
    a.sw = sw; a.sh = sh; a.sstride = sstride; a.fmt = fmt;
    a.dw = dw; a.dh = dh; a.dstride = dstride;
    a.tiles_x = (int32_t)grid_of(dw, RS_TW);
    const double ix = 1.0 / ((double)dw / sw), iy = 1.0 / ((double)dh / sh);
    a.dxl = (int64_t)(ix * 4294967296.0);
    a.dyl = (int64_t)(iy * 4294967296.0);
    a.x0l = (int64_t)(0.5 * ix * 4294967296.0);
    a.y0l = (int64_t)(0.5 * iy * 4294967296.0);
    return a;
}

int64_t resize_tiles(int dw, int dh) { return (int64_t)grid_of(dw, RS_TW) * grid_of(dh, RS_TH); }

// one image (descs == nullptr: `one` by value) or a batch of same-format images
static void launch_resize_fmt(int fmt, const ResizeArgs& one, const ResizeArgs* descs, const int64_t* prefix, int m,
                              dim3 grid, hipStream_t st)
{
    switch (fmt) {
    case ICX_GRAY8: ICX_LAUNCH((k_resize<1, 0, true>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_GRAY16: ICX_LAUNCH((k_resize<2, 0, true>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_INDEXED8: ICX_LAUNCH((k_resize<1, 0, false, 1>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_BINARY1: ICX_LAUNCH((k_resize<1, 0, false, 2>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_XRGB32: ICX_LAUNCH((k_resize<4, 3, true>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_ARGB32:
    case ICX_RGBA32: ICX_LAUNCH((k_resize<4, 3, false>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    case ICX_ABGR32: ICX_LAUNCH((k_resize<4, 0, false>), grid, dim3(256), 0, st, one, descs, prefix, m); break;
    default: ICX_LAUNCH((k_resize<3, 0, true>), grid, dim3(256), 0, st, one, descs, prefix, m);
    }
}

void launch_resize(const uint8_t* src, int sw, int sh, int sstride, int fmt, uint8_t* dst, int dw, int dh,
                   int dstride, hipStream_t st)
{
    launch_resize_one(resize_args(src, sw, sh, sstride, fmt, dst, dw, dh, dstride), st);
}

void launch_resize_one(const ResizeArgs& a, hipStream_t st)
{
    launch_resize_fmt(a.fmt, a, nullptr, nullptr, 1, dim3((unsigned)resize_tiles(a.dw, a.dh)), st);
}

void launch_resize_batch(int fmt, const ResizeArgs* descs, const int64_t* prefix, int m, int64_t tiles,
                         int64_t uniform, hipStream_t st)
{
    if (tiles <= 0) return;
    const dim3 grid = uniform > 0 && m > 1 ? dim3((unsigned)uniform, (unsigned)m) : dim3((unsigned)tiles);
    launch_resize_fmt(fmt, ResizeArgs{}, descs, prefix, m, grid, st);
}

}  // namespace icx
