// icx_pngfilter.hip — the per-row PNG filter of icx_png_encode on the device.
//
// What it restates (icx_png.cpp): convert_row / convert_pal_row (source bytes
// -> PNG sample order) and filter_row (RowFilter.filterRow: the five filters
// costed over the row with the bytes left of it and the row above the first
// reading as zero, the first strictly smaller cost wins), for every raster
// icx_png_encode accepts.  Output per image: height rows of 1 + n bytes, the
// exact bytes icx_png_encode hands to deflate.
//
// Layout.  One workgroup of 256 threads per (image, row); the launch covers
// a group of images of any sizes and formats (prefix of row counts, as the
// batched resize does with tiles).  A row is walked in tiles of PF_TILE PNG
// bytes.  Per tile the source bytes of the row and of the row above (which
// the workgroup of that row reads too: an L2 hit) are staged into LDS as they
// are, with 16-byte loads (the unaligned head and tail byte by byte; only
// bytes of the row are read); the conversion to sample order is an index
// computation on the LDS read, so the 3-byte pixel's left neighbour is one
// more LDS byte read at i - 3.  A thread owns one aligned dword of the
// output at a time: four consecutive residuals, stored as one dword (the
// row's first and last bytes singly - a row of 1 + n bytes starts anywhere).
// Pass 1 sums the five costs over all tiles of the row, pass 2 applies the
// winner; a row of one tile (up to PF_TILE bytes: a 1920-pixel RGB row)
// keeps its staged bytes between the passes, a wider one stages each tile
// again (L2).  Palette images (colour type 3) take filter 0 and skip pass 1.
//
// Costs are integers, so the reduction order cannot change the choice.  A
// thread's partial sums are 32 bits: it owns 4 bytes of every 1024, so at most
// n / 256 + 4 per tile bytes of a row of n <= 2^30 bytes (icx_png_bound's
// limit on the whole stream), times 255 < 2^31.  The sums over the workgroup
// are 64 bits.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "icx_internal.h"
#include "icx_pngfilter.h"

namespace icx {

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_TILE = 6144;  // PNG bytes per tile: a multiple of 12, so tiles start on pixels of 1-4 bytes
// source bytes of a tile and its one pixel to the left: XRGB32 is the widest
// (4 source bytes per 3), + 15 bytes of alignment slack
constexpr int PF_RAW = (PF_TILE / 3 + 1) * 4 + 16 + 12;

struct PfTile {
    int t0, len;   // PNG bytes [t0, t0 + len) of the row
    int rb;        // PNG byte index of the first staged pixel (t0 minus the left pixel)
    int raw_off;   // source byte offset of that pixel in the row
    int raw_len;   // staged source bytes
};

// global -> LDS, byte for byte; lds is 16-byte aligned and byte k of g lands
// at lds[pad + k], pad = g & 15, so whole 16-byte groups move as one load and
// one write.  Reads g[0 .. nbytes) only.
__device__ __forceinline__ int pf_stage(uint8_t* lds, const uint8_t* g, int nbytes)
{
    const int pad = (int)((uintptr_t)g & 15);
    const uint8_t* g0 = g - pad;
    const int total = pad + nbytes;
    const int nvec = (total + 15) >> 4;
    for (int v = threadIdx.x; v < nvec; v += PF_THREADS) {
        const int lo = v << 4, hi = lo + 16;
        if (lo >= pad && hi <= total) {
            *(uint4*)(lds + lo) = *(const uint4*)(g0 + lo);
        } else {
            const int b0 = lo > pad ? lo : pad, b1 = hi < total ? hi : total;
            for (int b = b0; b < b1; b++) lds[b] = g0[b];
        }
    }
    return pad;
}

// PNG sample r (counted from the first staged pixel) of a staged row.
template <int MODE>
__device__ __forceinline__ int pf_sample(const uint8_t* raw, int r, const PngFilterArgs& A, int pix0)
{
    if (MODE == PF_COPY) return raw[r];
    if (MODE == PF_SWAP16) return raw[r ^ 1];
    if (MODE == PF_ABGR32) return raw[r ^ 3];
    if (MODE == PF_ARGB32) return raw[(r & 3) == 3 ? r : r ^ ((r & 3) == 1 ? 0 : 2)];  // B, G, R, A -> R, G, B, A
    if (MODE == PF_BGR24 || MODE == PF_XRGB32) {
        const int q = r / 3, ch = r - 3 * q;
        return raw[(MODE == PF_BGR24 ? 3 : 4) * q + 2 - ch];
    }
    if (MODE == PF_PAL_GA) {
        const int idx = raw[r >> 1];
        const uint32_t c = A.pal[idx < A.pal_len ? idx : 0];
        return (int)((r & 1) ? c >> 24 : c & 255);
    }
    // PF_PACK: `per` pixels a byte, the first in the high bits
    const int per = 8 / A.depth, mask = (1 << A.depth) - 1;
    int v = 0;
    for (int k = 0; k < per; k++) {
        const int x = r * per + k;
        if (pix0 + x < A.w) v |= (raw[x] & mask) << (8 - A.depth * (k + 1));
    }
    return v;
}

__device__ __forceinline__ int pf_paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ PfTile pf_tile(const PngFilterArgs& A, int t0, int tile_len, int sb)
{
    PfTile T;
    T.t0 = t0;
    T.len = A.n - t0 < tile_len ? A.n - t0 : tile_len;
    int pix0, pix1;
    if (A.mode == PF_PACK) {
        const int per = 8 / A.depth;
        T.rb = t0 > 0 ? t0 - 1 : 0;
        pix0 = T.rb * per;
        pix1 = (t0 + T.len) * per < A.w ? (t0 + T.len) * per : A.w;
    } else {
        pix0 = t0 / A.bpp - (t0 > 0 ? 1 : 0);
        pix1 = (t0 + T.len) / A.bpp;
        T.rb = pix0 * A.bpp;
    }
    T.raw_off = pix0 * sb;
    T.raw_len = (pix1 - pix0) * sb;
    return T;
}

// One pass over a staged tile.  APPLY = false: adds the tile's five costs to
// cost[]; APPLY = true: writes the residuals of filter `best` to og[0 .. len).
template <int MODE, bool APPLY>
__device__ __forceinline__ void pf_pass(const PngFilterArgs& A, const PfTile& T, const uint8_t* cur,
                                        const uint8_t* prev, bool has_prev, uint8_t* og, int best, uint32_t cost[5])
{
    const int pix0 = A.mode == PF_PACK ? T.rb * (8 / A.depth) : 0;
    const int opad = (int)((uintptr_t)og & 3);
    const int nd = (opad + T.len + 3) >> 2;
    const int bpp = A.bpp;
    for (int q = threadIdx.x; q < nd; q += PF_THREADS) {
        uint32_t word = 0;
        const int j0 = 4 * q - opad;
        for (int k = 0; k < 4; k++) {
            const int j = j0 + k;
            if (j < 0 || j >= T.len) continue;
            const int i = T.t0 + j, r = i - T.rb;
            const bool left = i >= bpp;
            const int x = pf_sample<MODE>(cur, r, A, pix0);
            const int a = left ? pf_sample<MODE>(cur, r - bpp, A, pix0) : 0;
            const int b = has_prev ? pf_sample<MODE>(prev, r, A, pix0) : 0;
            const int c = has_prev && left ? pf_sample<MODE>(prev, r - bpp, A, pix0) : 0;
            if (!APPLY) {
                cost[0] += (uint32_t)x;
                cost[1] += (uint32_t)abs(x - a);
                cost[2] += (uint32_t)abs(x - b);
                cost[3] += (uint32_t)abs(x - ((a + b) >> 1));
                cost[4] += (uint32_t)abs(x - pf_paeth(a, b, c));
            } else {
                const int p = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? (a + b) >> 1 : pf_paeth(a, b, c);
                word |= (uint32_t)((x - p) & 255) << (8 * k);
            }
        }
        if (APPLY) {
            if (j0 >= 0 && j0 + 4 <= T.len) {
                *(uint32_t*)(og + j0) = word;
            } else {
                for (int k = 0; k < 4; k++)
                    if (j0 + k >= 0 && j0 + k < T.len) og[j0 + k] = (uint8_t)(word >> (8 * k));
            }
        }
    }
}

template <int MODE>
__device__ __forceinline__ void pf_row(const PngFilterArgs& A, int y, uint8_t* s_cur, uint8_t* s_prev,
                                       unsigned long long (*s_cost)[5])
{
    const int sb = MODE == PF_COPY ? A.bpp : MODE == PF_SWAP16 ? 2 : MODE == PF_BGR24 ? 3
                   : MODE == PF_PAL_GA || MODE == PF_PACK ? 1 : 4;
    const int tile_len = MODE == PF_PACK ? PF_TILE / (8 / A.depth) : PF_TILE;
    const uint8_t* row = A.src + (size_t)y * A.sstride;
    const bool has_prev = y > 0;
    uint8_t* out = A.out + (size_t)y * ((size_t)A.n + 1);
    const bool one = A.n <= tile_len;
    int best = 0;
    int cpad = 0, ppad = 0;
    if (!A.force0) {
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int t0 = 0; t0 < A.n; t0 += tile_len) {
            const PfTile T = pf_tile(A, t0, tile_len, sb);
            if (t0 > 0) __syncthreads();  // the tile before is read out
            cpad = pf_stage(s_cur, row + T.raw_off, T.raw_len);
            if (has_prev) ppad = pf_stage(s_prev, row - A.sstride + T.raw_off, T.raw_len);
            __syncthreads();
            pf_pass<MODE, false>(A, T, s_cur + cpad, s_prev + ppad, has_prev, nullptr, 0, cost);
        }
        unsigned long long tot[5];
        for (int f = 0; f < 5; f++) {
            unsigned long long v = cost[f];
            for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
            tot[f] = v;
        }
        if ((threadIdx.x & 63) == 0)
            for (int f = 0; f < 5; f++) s_cost[threadIdx.x >> 6][f] = tot[f];
        __syncthreads();
        for (int f = 0; f < 5; f++) {
            tot[f] = 0;
            for (int w = 0; w < PF_THREADS / 64; w++) tot[f] += s_cost[w][f];
        }
        for (int f = 1; f < 5; f++)
            if (tot[f] < tot[best]) best = f;  // the first strictly smaller cost: ties keep the lower type
    }
    for (int t0 = 0; t0 < A.n; t0 += tile_len) {
        const PfTile T = pf_tile(A, t0, tile_len, sb);
        if (A.force0 || !one) {
            __syncthreads();
            cpad = pf_stage(s_cur, row + T.raw_off, T.raw_len);
            if (has_prev && best >= 2) ppad = pf_stage(s_prev, row - A.sstride + T.raw_off, T.raw_len);
            __syncthreads();
        }
        uint32_t none[5];
        pf_pass<MODE, true>(A, T, s_cur + cpad, s_prev + ppad, has_prev && best >= 2, out + 1 + t0, best, none);
    }
    if (threadIdx.x == 0) out[0] = (uint8_t)best;
}

// Launch slot of a row: prefix[lo] <= item < prefix[lo + 1].
__device__ __forceinline__ int pf_slot(const int64_t* prefix, int m, int64_t item)
{
    int lo = 0, hi = m;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PF_THREADS) void k_png_filter(const PngFilterArgs* __restrict__ descs,
                                                           const int64_t* __restrict__ prefix, int m)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_cur[PF_RAW];
    __shared__ __attribute__((aligned(16))) uint8_t s_prev[PF_RAW];
    __shared__ unsigned long long s_cost[PF_THREADS / 64][5];
    const int64_t item = blockIdx.x;
    const int slot = pf_slot(prefix, m, item);
    const PngFilterArgs A = descs[slot];
    const int y = (int)(item - prefix[slot]);
    switch (A.mode) {
    case PF_COPY: pf_row<PF_COPY>(A, y, s_cur, s_prev, s_cost); break;
    case PF_SWAP16: pf_row<PF_SWAP16>(A, y, s_cur, s_prev, s_cost); break;
    case PF_BGR24: pf_row<PF_BGR24>(A, y, s_cur, s_prev, s_cost); break;
    case PF_XRGB32: pf_row<PF_XRGB32>(A, y, s_cur, s_prev, s_cost); break;
    case PF_ARGB32: pf_row<PF_ARGB32>(A, y, s_cur, s_prev, s_cost); break;
    case PF_ABGR32: pf_row<PF_ABGR32>(A, y, s_cur, s_prev, s_cost); break;
    case PF_PAL_GA: pf_row<PF_PAL_GA>(A, y, s_cur, s_prev, s_cost); break;
    default: pf_row<PF_PACK>(A, y, s_cur, s_prev, s_cost);
    }
}

}  // namespace

void launch_png_filter(const PngFilterArgs* descs, const int64_t* prefix, int m, int64_t rows, hipStream_t st)
{
    if (rows <= 0) return;
    LaunchTiming& lt = g_launch_timing;
    if (lt.a) {  // a Timed region's events: recorded at the dispatch's start and end
        hipExtLaunchKernelGGL(k_png_filter, dim3((unsigned)rows), dim3(PF_THREADS), 0, st, lt.a, lt.b, 0, descs,
                              prefix, m);
        lt.a = lt.b = nullptr;
        lt.used = true;
    } else {
        hipLaunchKernelGGL(k_png_filter, dim3((unsigned)rows), dim3(PF_THREADS), 0, st, descs, prefix, m);
    }
}

}  // namespace icx
