// batch.hip — nabu_batch_unpack: one packed batch buffer -> every padded tensor of the batch contract, in one launch.
//
// The host packs a batch without its padding (processing/prefetch.py: per tensor B lengths, B + 1 row offsets, the rows
// back to back), uploads it with ONE copy and this kernel writes [rows, max_len, width] per tensor: data where
// t < len[b], zero elsewhere, plus the length vector.  A copy kernel: no LDS, no communication between workgroups, a
// capped grid that strides over the output elements of all segments.
//
// Access widths: a segment whose width is a multiple of 4 moves 16 bytes per lane (its row offsets are then multiples
// of 4 elements and the row data starts 16-byte aligned, so every load and store is aligned); any other width (label
// vectors, the 123-column features) moves 4 bytes per lane.  Consecutive lanes touch consecutive addresses in both.
//
// Bounds: len[b] is clamped to [0, max_len] before it is used and a row whose offsets leave the segment's data region
// is written as zeros, so a corrupt header can make the result wrong but can neither read nor write out of bounds.
#include "common.h"

namespace nabu {

struct UnpackSeg {
  const int32_t *len;       // [rows]
  const int32_t *row_off;   // [rows + 1] element offsets into data
  const uint32_t *data;     // 4-byte elements, 16-byte aligned
  uint32_t *out;            // [rows, max_len, width]
  int32_t *out_len;         // [rows]
  unsigned cap;             // elements of the packed buffer behind data
  unsigned row_items;       // work items of one output row: max_len * width (/ 4 when vec)
  int rows, width, max_len, vec;
};

struct UnpackArgs {
  UnpackSeg seg[NABU_BATCH_MAX_SEGS];
  unsigned long long first[NABU_BATCH_MAX_SEGS + 1];   // first work item of every segment; first[n] = all of them
  int n;
};

__global__ __launch_bounds__(256) void batch_unpack_kernel(const UnpackArgs a) {
  const unsigned long long total = a.first[a.n];
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int s = 0;
    while (s + 1 < a.n && i >= a.first[s + 1]) ++s;
    const UnpackSeg &g = a.seg[s];
    const unsigned local = (unsigned)(i - a.first[s]);         // < 2^31 (checked by the host)
    const unsigned b = local / g.row_items, r = local - b * g.row_items;
    int len = g.len[b];
    len = len < 0 ? 0 : (len > g.max_len ? g.max_len : len);
    if (r == 0) g.out_len[b] = len;
    const unsigned valid = (unsigned)len * (unsigned)g.width;  // elements of row b that hold data
    const long long off = g.row_off[b];
    const bool inside = off >= 0 && (unsigned long long)off + valid <= g.cap;
    if (g.vec) {
      const unsigned e = 4u * r;                                // width % 4 == 0: a group is all data or all padding
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (e < valid && inside && (off & 3) == 0) v = *reinterpret_cast<const uint4 *>(g.data + off + e);
      *reinterpret_cast<uint4 *>(g.out + (size_t)local * 4) = v;
    } else {
      g.out[local] = (r < valid && inside) ? g.data[off + r] : 0u;
    }
  }
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_batch_unpack(int nseg, const nabu_batch_seg *segs_host, const void *packed_dev, size_t packed_bytes,
                                 nabu_stream_t stream) {
  NABU_CHECK_ARG(segs_host && packed_dev, "batch_unpack: null pointer");
  NABU_CHECK_ARG(nseg >= 1 && nseg <= NABU_BATCH_MAX_SEGS, "batch_unpack: nseg = %d is outside 1..%d", nseg,
                 NABU_BATCH_MAX_SEGS);
  NABU_CHECK_ARG((uintptr_t)packed_dev % 16 == 0, "batch_unpack: the packed buffer must be 16-byte aligned");
  const char *base = static_cast<const char *>(packed_dev);
  UnpackArgs a = {};
  a.n = nseg;
  for (int s = 0; s < nseg; ++s) {
    const nabu_batch_seg &h = segs_host[s];
    NABU_CHECK_ARG(h.rows > 0 && h.width > 0 && h.max_len > 0, "batch_unpack: segment %d: rows, width and max_len must be positive", s);
    NABU_CHECK_ARG(h.out && h.out_len, "batch_unpack: segment %d: null output", s);
    const unsigned long long elems = (unsigned long long)h.rows * h.max_len * h.width;
    NABU_CHECK_ARG(elems < (1ull << 31), "batch_unpack: segment %d holds 2^31 elements or more", s);
    NABU_CHECK_ARG(h.len_off % 4 == 0 && h.row_off % 4 == 0 && h.data_off % 16 == 0,
                   "batch_unpack: segment %d: misaligned offset", s);
    NABU_CHECK_ARG((uintptr_t)h.out % 4 == 0 && (uintptr_t)h.out_len % 4 == 0, "batch_unpack: segment %d: misaligned output", s);
    const size_t lens = 4 * (size_t)h.rows;
    NABU_CHECK_ARG(h.len_off <= packed_bytes && lens <= packed_bytes - h.len_off &&
                   h.row_off <= packed_bytes && lens + 4 <= packed_bytes - h.row_off && h.data_off <= packed_bytes,
                   "batch_unpack: segment %d lies outside the %zu packed bytes", s, packed_bytes);
    UnpackSeg &g = a.seg[s];
    g.len = reinterpret_cast<const int32_t *>(base + h.len_off);
    g.row_off = reinterpret_cast<const int32_t *>(base + h.row_off);
    g.data = reinterpret_cast<const uint32_t *>(base + h.data_off);
    g.out = static_cast<uint32_t *>(h.out);
    g.out_len = h.out_len;
    const size_t cap = (packed_bytes - h.data_off) / 4;
    g.cap = cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)cap;
    g.rows = h.rows, g.width = h.width, g.max_len = h.max_len;
    g.vec = h.width % 4 == 0 && (uintptr_t)h.out % 16 == 0;
    g.row_items = (unsigned)h.max_len * (unsigned)h.width / (g.vec ? 4u : 1u);
    a.first[s + 1] = a.first[s] + (unsigned long long)h.rows * g.row_items;
  }
  unsigned long long blocks = (a.first[nseg] + 255) / 256;
  if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 blocks, the loop strides over the rest
  hipLaunchKernelGGL(batch_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  NABU_LAUNCH_CHECK();
  return 0;
}
