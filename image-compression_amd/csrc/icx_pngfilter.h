// icx_pngfilter.h — the PNG row filter on the device (icx_pngfilter.hip) and
// the host description of a raster's PNG rows (icx_png.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/icx.h"

namespace icx {

// How a source row becomes PNG samples (convert_row / convert_pal_row of
// icx_png.cpp): PNG byte i of pixel q = i / bpp, channel ch = i % bpp reads
enum PngFilterMode {
    PF_COPY = 0,    // source byte i (GRAY8, RGB24, RGBA32, 8-bit palette indices / grey levels)
    PF_SWAP16 = 1,  // GRAY16: i ^ 1 (little-endian samples -> big-endian)
    PF_BGR24 = 2,   // 3q + 2 - ch
    PF_XRGB32 = 3,  // 4q + 2 - ch (bytes B, G, R, X -> R, G, B)
    PF_ARGB32 = 4,  // 4q + (2 - ch, alpha in place) (bytes B, G, R, A)
    PF_ABGR32 = 5,  // 4q + 3 - ch (bytes A, B, G, R)
    PF_PAL_GA = 6,  // grey-ramp map with alpha: map[index] -> grey, alpha
    PF_PACK = 7     // 1/2/4-bit indices, packed MSB first
};

// One image of a launch.  `out` receives h rows of 1 + n bytes: the filter
// type, then the residuals.
struct PngFilterArgs {
    const uint8_t* src;   // device pixels, rows of sstride bytes
    uint8_t* out;         // device, h * (n + 1) bytes
    const uint32_t* pal;  // device colour map, 256 entries (PF_PAL_GA), else unused
    int32_t w, h, sstride, mode;
    int32_t n;        // PNG row bytes
    int32_t bpp;      // RowFilter's bytesPerPixel
    int32_t depth;    // bits per sample of a PF_PACK row
    int32_t force0;   // palette image (colour type 3): filter 0 on every row
    int32_t pal_len;  // entries of the colour map (indices past it read entry 0)
    int32_t pad_;
};

// Fills mode, n, bpp, depth, force0 and pal_len from the raster (w, h, fmt,
// palette; px is not read): the choices icx_png_encode makes for it.
void png_filter_desc(const icx_image* img, PngFilterArgs* a);

// m descriptors in device memory, prefix = exclusive row counts (prefix[m] =
// rows): one workgroup per (image, row).
void launch_png_filter(const PngFilterArgs* descs, const int64_t* prefix, int m, int64_t rows, hipStream_t st);

}  // namespace icx
