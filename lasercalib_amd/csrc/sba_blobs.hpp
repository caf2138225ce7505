// sba_blobs.hpp -- sba_detect_blobs (include/sba_hip.h): the careful laser-dot detector of the reference, green_laser_finder
// (lasercalib/feature_detection.py:6-40): threshold, binary_dilation(disk(1)), binary_closing(disk(4)), measure.label,
// regionprops, "exactly one connected component".  DESIGN.md 4.10 has the passes, the memory and the visibility argument.
//
// Per chunk of frames, all on one stream:
//   k_blob_init       the blob table: sums = 0, xmin = ymin = all ones
//   k_blob_threshold  the ONLY pass over the frame bytes (read as k_dot_moments reads them: scan_row of sba_frames.hpp, which
//                     also has the chunks and the staging of host frames): the raw mask, one bit per pixel in 64-pixel words,
//                     and the value byte of every raw pixel
//   k_blob_morph      dilation by disk(r1) (+) disk(r2), then erosion by disk(r2), on words: shifts with carries between
//                     neighbouring words, a band of rows plus a halo of r1 + 2 r2 rows staged in LDS
//   k_blob_label_tile union-find of the pixels of one 32 x 64 tile in LDS; label = smallest linear index y W + x of the tree
//   k_blob_merge      unions across tile borders: agent-scope atomicMin / relaxed atomic loads only, no waiting
//   k_blob_flatten    every pixel points at its root; roots are counted per row
//   k_blob_prefix     exclusive prefix of the row counts: the rank of a row's first root; their total = n_components
//   k_blob_rank       a root's label becomes -(rank + 1): raster order of the roots is the order of measure.label
//   k_blob_stats      the 12 integers of every listed component, pre-reduced per wave, merged with integer atomics
//   k_blob_expand     (diagnostics only) the mask as bytes, the labels as 1, 2, ...
// Everything after the threshold pass reads bit words (1/8 .. 1/32 of the frame's bytes) and skips all-zero words and tiles;
// labels and value bytes exist only where a mask bit is set and are never initialised elsewhere.
#pragma once
#include "sba_detect.hpp"

namespace sba_detect {

constexpr int BLOB_MAX_RADIUS = 8;
constexpr int BLOB_MAX_DH = 2 * BLOB_MAX_RADIUS;          // rows the composed dilation reaches
constexpr int BLOB_NREC = 12;                             // n, sx, sy, n_raw, sw, swx, swy, n_sat, xmin, ymin, xmax, ymax
constexpr int BLOB_MAX_BLOBS = 64, BLOB_DEFAULT_BLOBS = 8;
constexpr int MORPH_ROWS = 32, MORPH_WORDS = 8, MORPH_THREADS = 256;      // a workgroup's band: 32 rows x 512 pixels
constexpr int TILE_ROWS = 32, TILE_THREADS = 256;         // labelling tile: TILE_ROWS rows x 64 pixels (one word column)
constexpr int TILE_STRIP = TILE_THREADS / TILE_ROWS;      // tiles side by side that one workgroup loads and, where set, labels
constexpr int BLOB_WAVE_WORDS = 256;                      // words one wave of flatten / stats walks, 64 (a lane each) at a time
constexpr int64_t BLOB_SCRATCH_BYTES = (int64_t)1 << 30;  // budget of the per-frame scratch of one chunk; one frame always fits

typedef unsigned long long u64;

struct BlobParams : FrameView {
  int32_t rows_per_band;
  int32_t ww;                                // 64-pixel words of one row
  int32_t dh, eh;                            // rows the composed dilation / the erosion reach
  int8_t hwd[BLOB_MAX_DH + 1];               // half-width of the composed dilation's row |dy|; -1 = no such row
  int8_t hwe[BLOB_MAX_RADIUS + 1];           // the same of the erosion's disk
  int32_t max_blobs, want_labels;
};

// the per-frame scratch of a chunk; frame f starts at f times the stride given
struct BlobScratch {
  u64 *raw, *mask;                           // H ww words each
  uint8_t* vals;                             // H W: the value byte, written where raw is set
  int* lab;                                  // H W: written where mask is set
  int *rowcnt, *rowbase;                     // H
  int* ncomp;                                // 1
  u64* table;                                // max_blobs BLOB_NREC
};

// Row half-widths of disk(r): floor(sqrt(r^2 - d^2)).  Dilating by disk(r1) and then by disk(r2) is ONE dilation by their
// Minkowski sum: its row dy is the union of the intervals [-(hw1 + hw2), hw1 + hw2] over dy1 + dy2 = dy, all centred on 0, so
// the widest one.  (The cropping of the first result to the frame loses nothing: a path p -> p + a -> p + a + b that leaves the
// frame at p + a has the path through clamp(p + a), whose two steps are component-wise no longer.)
inline void blob_halfwidths(int r1, int r2, int8_t* hwd, int8_t* hwe) {
  auto hw = [](int r, int d) { int h = 0; while ((h + 1) * (h + 1) + d * d <= r * r) ++h; return h; };
  for (int d = 0; d <= BLOB_MAX_DH; ++d) hwd[d] = -1;
  for (int d1 = -r1; d1 <= r1; ++d1)
    for (int d2 = -r2; d2 <= r2; ++d2) {
      const int d = std::abs(d1 + d2);
      hwd[d] = (int8_t)std::max<int>(hwd[d], hw(r1, std::abs(d1)) + hw(r2, std::abs(d2)));
    }
  for (int d = 0; d <= BLOB_MAX_RADIUS; ++d) hwe[d] = (int8_t)(d <= r2 ? hw(r2, d) : -1);
}

__global__ void k_blob_init(u64* __restrict__ table, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = (int)(i % BLOB_NREC);
  table[i] = k == 8 || k == 9 ? ~0ull : 0ull;
}

// ------------------------------------------------------------------------------------------------ threshold
// scan_row's sink: sets the bit of every pixel above the threshold in the wave's LDS row and stores its value byte
struct BlobSink {
  uint32_t* row32;
  uint8_t* __restrict__ vrow;
  uint32_t thr;
  template <int NPIX>
  __device__ __forceinline__ void operator()(uint32_t xq, const uint32_t (&v)[NPIX]) {
#pragma unroll
    for (int k = 0; k < NPIX; ++k)
      if (v[k] > thr) {
        const uint32_t x = xq + (uint32_t)k;
        atomicOr(&row32[x >> 5], 1u << (x & 31u));
        vrow[x] = (uint8_t)v[k];
      }
  }
};

// grid (bands, frames), DOT_THREADS threads; wave w takes rows band_lo + w, + w + 4, ... of ALL rows of the frame (a row outside
// the regions gets zero words).  The bits of a row are gathered in the wave's own LDS row, which is all zero between rows.
template <int C>
__global__ void __launch_bounds__(DOT_THREADS) k_blob_threshold(const BlobParams P, u64* __restrict__ raw, uint8_t* __restrict__ vals) {
  __shared__ u64 s_row[DOT_WAVES][DOT_MAX_DIM / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y;
  const uint32_t thr = (uint32_t)P.threshold, channel = (uint32_t)P.channel;
  const int band_lo = (int)blockIdx.x * P.rows_per_band;
  const int band_hi = min(P.height, band_lo + P.rows_per_band);
  const uint8_t* __restrict__ fp = P.frames + (int64_t)f * P.frame_pitch;
  u64* myrow = s_row[wave];
  for (int i = lane; i < P.ww; i += 64) myrow[i] = 0;
  wave_lds_sync();

  for (int y = band_lo + wave; y < band_hi; y += DOT_WAVES) {
    u64* __restrict__ out = raw + ((size_t)f * P.height + y) * P.ww;
    BlobSink S{reinterpret_cast<uint32_t*>(myrow), vals + ((size_t)f * P.height + y) * P.width, thr};
    int xa, xb;
    const bool hit = frame_row_span(P, y, xa, xb) && scan_row<C>(fp + (int64_t)y * P.row_pitch, xa, xb, channel, thr, S);
    if (!hit) {                                                          // the usual case: a dark row
      for (int i = lane; i < P.ww; i += 64) out[i] = 0;
      continue;
    }
    wave_lds_sync();
    for (int i = lane; i < P.ww; i += 64) { out[i] = myrow[i]; myrow[i] = 0; }
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------------------------ morphology
// Bit b of word i is pixel x = 64 i + b: `c << s` moves pixels to larger x, and the top bits of the left neighbour come in below.
__device__ __forceinline__ u64 blob_hdilate(u64 l, u64 c, u64 r, int hw) {
  u64 o = c;
  for (int s = 1; s <= hw; ++s) o |= (c << s) | (l >> (64 - s)) | (c >> s) | (r << (64 - s));
  return o;
}
__device__ __forceinline__ u64 blob_herode(u64 l, u64 c, u64 r, int hw) {
  u64 o = c;
  for (int s = 1; s <= hw; ++s) o &= ((c << s) | (l >> (64 - s))) & ((c >> s) | (r << (64 - s)));
  return o;
}

// grid (word tiles, bands, frames).  LDS: the raw words of the band's rows +- (dh + eh) and of one word column either side (the
// composed dilation and the erosion together reach dh + eh <= 24 < 64 pixels sideways), then the dilated words of the rows +- eh.
// Outside the frame the dilation reads 0 and the erosion reads 1 (skimage's mode='ignore'): the dilated image is all ones there.
// A dilated word of a halo column is right only in the eh <= 8 bits next to the band, which is all the erosion reads of it.
__global__ void __launch_bounds__(MORPH_THREADS) k_blob_morph(const BlobParams P, const u64* __restrict__ raw, u64* __restrict__ mask) {
  constexpr int CW = MORPH_WORDS + 2;
  constexpr int RR = MORPH_ROWS + 2 * (BLOB_MAX_DH + BLOB_MAX_RADIUS), DR = MORPH_ROWS + 2 * BLOB_MAX_RADIUS;
  __shared__ u64 s_raw[RR][CW], s_dil[DR][CW];
  const int t = threadIdx.x, f = blockIdx.z;
  const int y0 = (int)blockIdx.y * MORPH_ROWS, w0 = (int)blockIdx.x * MORPH_WORDS;
  const int H = P.height, W = P.width, ww = P.ww, dh = P.dh, eh = P.eh, halo = dh + eh;
  const u64* __restrict__ rf = raw + (size_t)f * H * ww;
  u64* __restrict__ mf = mask + (size_t)f * H * ww;
  const u64 beyond = (W & 63) ? ~0ull << (W & 63) : 0ull;               // the bits of the row's last word that are no pixels

  int any = 0;
  for (int i = t; i < (MORPH_ROWS + 2 * halo) * CW; i += MORPH_THREADS) {
    const int rr = i / CW, c = i - rr * CW, y = y0 - halo + rr, wi = w0 - 1 + c;
    const u64 v = (y >= 0 && y < H && wi >= 0 && wi < ww) ? rf[(size_t)y * ww + wi] : 0ull;
    s_raw[rr][c] = v;
    any |= v != 0;
  }
  if (!__syncthreads_or(any)) {              // nothing raw within reach: every pixel of the band erodes to 0 (its own dilated bit is 0)
    for (int i = t; i < MORPH_ROWS * MORPH_WORDS; i += MORPH_THREADS) {
      const int r = i / MORPH_WORDS, y = y0 + r, wi = w0 + (i - r * MORPH_WORDS);
      if (y < H && wi < ww) mf[(size_t)y * ww + wi] = 0;
    }
    return;
  }
  for (int i = t; i < (MORPH_ROWS + 2 * eh) * CW; i += MORPH_THREADS) {
    const int r = i / CW, c = i - r * CW, y = y0 - eh + r, wi = w0 - 1 + c;
    u64 d = ~0ull;
    if (y >= 0 && y < H && wi >= 0 && wi < ww) {
      d = 0;
      for (int dy = -dh; dy <= dh; ++dy) {
        const int hw = P.hwd[dy < 0 ? -dy : dy], rr = r + dh + dy;
        if (hw < 0) continue;
        const u64 l = c > 0 ? s_raw[rr][c - 1] : 0ull, m = s_raw[rr][c], rt = c < CW - 1 ? s_raw[rr][c + 1] : 0ull;
        if (l | m | rt) d |= blob_hdilate(l, m, rt, hw);
      }
      if (wi == ww - 1) d |= beyond;
    }
    s_dil[r][c] = d;
  }
  __syncthreads();
  for (int i = t; i < MORPH_ROWS * MORPH_WORDS; i += MORPH_THREADS) {
    const int r = i / MORPH_WORDS, c = 1 + (i - r * MORPH_WORDS), y = y0 + r, wi = w0 - 1 + c;
    if (y >= H || wi >= ww) continue;
    u64 e = ~0ull;
    for (int dy = -eh; dy <= eh; ++dy) {
      const int hw = P.hwe[dy < 0 ? -dy : dy], row = r + eh + dy;
      if (hw < 0) continue;
      e &= blob_herode(s_dil[row][c - 1], s_dil[row][c], s_dil[row][c + 1], hw);
    }
    if (wi == ww - 1) e &= ~beyond;
    mf[(size_t)y * ww + wi] = e;
  }
}

// ------------------------------------------------------------------------------------------------ labelling
// Union-find with "the parent is never larger than the child": the root of a tree is its smallest index, and every chain of
// parents strictly descends, so every loop below ends after at most as many steps as the tree is deep.
__device__ __forceinline__ int blob_lds_find(int* lab, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void blob_lds_union(int* lab, int a, int b) {
  for (;;) {
    a = blob_lds_find(lab, a); b = blob_lds_find(lab, b);
    if (a == b) return;
    if (a > b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(&lab[b], a);   // b was a root when read; if it no longer is, `old` is its parent: go on from there
    if (old == b) return;
    b = old;
  }
}

// grid (ceil(ww / TILE_STRIP), tile rows, frames).  The workgroup loads the words of TILE_STRIP tiles side by side, a thread
// each, and labels those that hold a pixel, one after the other.  A pixel starts at the first pixel of its horizontal run
// inside the word, is united with the runs of the row above that touch it (8-connectivity: N, NW, NE), and ends pointing at
// the tile-local root, as a frame index.
__global__ void __launch_bounds__(TILE_THREADS) k_blob_label_tile(const BlobParams P, const u64* __restrict__ mask, int* __restrict__ lab) {
  __shared__ u64 s_mm[TILE_STRIP][TILE_ROWS + 1];
  __shared__ int s_any[TILE_STRIP];
  __shared__ int s_lab[TILE_ROWS * 64];
  const int t = threadIdx.x, b = t & 63, wave = t >> 6;
  const int ty0 = (int)blockIdx.y * TILE_ROWS, f = blockIdx.z;
  const int H = P.height, W = P.width, ww = P.ww;
  {
    const int r = t / TILE_STRIP, c = t - r * TILE_STRIP, wi = (int)blockIdx.x * TILE_STRIP + c;
    u64 w = 0;
    if (ty0 + r < H && wi < ww) w = mask[((size_t)f * H + ty0 + r) * ww + wi];
    if (!__syncthreads_or(w != 0)) return;                               // the usual case: a dark strip
    s_mm[c][r + 1] = w;
    if (t < TILE_STRIP) { s_mm[t][0] = 0; s_any[t] = 0; }
    __syncthreads();
    if (w) s_any[c] = 1;
    __syncthreads();
  }
  int* __restrict__ lf = lab + (size_t)f * H * W;
  for (int c = 0; c < TILE_STRIP; ++c) {
    if (!s_any[c]) continue;                                             // the same for every thread
    const u64* s_m = s_mm[c];
    const int wi = (int)blockIdx.x * TILE_STRIP + c;
    for (int r = wave; r < TILE_ROWS; r += TILE_THREADS / 64) {
      const u64 m = s_m[r + 1];
      if ((m >> b) & 1) {
        const u64 low = ~m & ((1ull << b) - 1);                          // the unset pixels below b
        s_lab[r * 64 + b] = r * 64 + (low ? 64 - __clzll((long long)low) : 0);
      }
    }
    __syncthreads();
    for (int r = wave; r < TILE_ROWS; r += TILE_THREADS / 64) {
      const u64 m = s_m[r + 1], up = s_m[r];
      if (!((m >> b) & 1) || up == 0) continue;
      const bool n = (up >> b) & 1, nw = b > 0 && ((up >> (b - 1)) & 1), ne = b < 63 && ((up >> (b + 1)) & 1);
      const bool wst = b > 0 && ((m >> (b - 1)) & 1);
      const int i = r * 64 + b;
      if (n) { if (!(wst && nw)) blob_lds_union(s_lab, i, i - 64); }     // else the pixel to the west has united the two runs
      else {
        if (nw && !wst) blob_lds_union(s_lab, i, i - 65);
        if (ne) blob_lds_union(s_lab, i, i - 63);
      }
    }
    __syncthreads();
    for (int r = wave; r < TILE_ROWS; r += TILE_THREADS / 64) {
      if (!((s_m[r + 1] >> b) & 1)) continue;
      const int root = blob_lds_find(s_lab, r * 64 + b);
      lf[(ty0 + r) * W + wi * 64 + b] = (ty0 + (root >> 6)) * W + wi * 64 + (root & 63);
    }
    __syncthreads();                                                     // s_lab is free for the next tile
  }
}

// Labels that another workgroup of the SAME launch may read or write: every read is an agent-scope relaxed atomic load, every
// write an agent-scope atomicMin (never a plain store, which could sit in this CU's cache), and the union acts on the value the
// atomicMin RETURNS, not on what it read before.  A stale read therefore costs a step, never the result.
__device__ __forceinline__ int blob_find(int* lab, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void blob_union(int* lab, int a, int b) {
  for (;;) {
    a = blob_find(lab, a); b = blob_find(lab, b);
    if (a == b) return;
    if (a > b) { const int s = a; a = b; b = s; }
    const int old = __hip_atomic_fetch_min(&lab[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) return;
    b = old;
  }
}
__device__ __forceinline__ bool blob_bit(const u64* __restrict__ mf, int ww, int H, int W, int y, int x) {
  if (y < 0 || y >= H || x < 0 || x >= W) return false;
  return (mf[(size_t)y * ww + (x >> 6)] >> (x & 63)) & 1;
}

// grid (ceil(H ww / 256), frames), a thread per word.  Two 8-adjacent pixels of different tiles are either in different tile
// rows -- then the lower one is in the top row of its tile and the other is its N, NW or NE -- or in the same tile row and
// neighbouring word columns -- then the right one is bit 0 of its word and the other is its W, NW or SW.  The first kind is
// worked off by the whole wave, a lane per pixel of the word; the second by the word's own thread.
__global__ void __launch_bounds__(256) k_blob_merge(const BlobParams P, const u64* __restrict__ mask, int* __restrict__ lab) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const int H = P.height, W = P.width, ww = P.ww;
  const int64_t total = (int64_t)H * ww, mine = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const u64* __restrict__ mf = mask + (size_t)f * H * ww;
  int* lf = lab + (size_t)f * H * W;
  const u64 ml = mine < total ? mf[mine] : 0ull;
  const int y = (int)(mine / ww), wi = (int)(mine - (int64_t)y * ww);
  if ((ml & 1) && wi > 0) {
    const int x = wi * 64;
    for (int k = 0; k < 3; ++k)
      if (blob_bit(mf, ww, H, W, y - 1 + k, x - 1)) blob_union(lf, y * W + x, (y - 1 + k) * W + x - 1);
  }
  u64 nz = __ballot(ml != 0 && y > 0 && y % TILE_ROWS == 0);
  while (nz) {
    const int j = __ffsll((long long)nz) - 1;
    nz &= nz - 1;
    const u64 m = __shfl(ml, j, 64);
    const int yy = __shfl(y, j, 64), x = __shfl(wi, j, 64) * 64 + lane;
    if ((m >> lane) & 1)
      for (int k = 0; k < 3; ++k)
        if (blob_bit(mf, ww, H, W, yy - 1, x - 1 + k)) blob_union(lf, yy * W + x, (yy - 1) * W + x - 1 + k);
  }
}

// grid (ceil(H ww / (4 BLOB_WAVE_WORDS)), frames): a wave loads 64 words at a time, a lane each, and works off those that hold
// a pixel, a lane per pixel.  No union runs in this launch, so the roots are fixed; a pixel's label is overwritten with an
// ancestor of it, which is what any other lane may read of it.
__global__ void __launch_bounds__(256) k_blob_flatten(const BlobParams P, const u64* __restrict__ mask, int* __restrict__ lab, int* __restrict__ rowcnt) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const int H = P.height, W = P.width, ww = P.ww;
  const int64_t total = (int64_t)H * ww;
  const int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * BLOB_WAVE_WORDS;
  const u64* __restrict__ mf = mask + (size_t)f * H * ww;
  int* lf = lab + (size_t)f * H * W;
  for (int64_t base = w0; base < min(total, w0 + BLOB_WAVE_WORDS); base += 64) {
    const u64 ml = base + lane < total ? mf[base + lane] : 0ull;
    u64 nz = __ballot(ml != 0);
    while (nz) {
      const int j = __ffsll((long long)nz) - 1;
      nz &= nz - 1;
      const u64 m = __shfl(ml, j, 64);
      const int64_t s = base + j;
      const int y = (int)(s / ww), wi = (int)(s - (int64_t)y * ww);
      bool root = false;
      if ((m >> lane) & 1) {
        const int p = y * W + wi * 64 + lane, r = blob_find(lf, p);
        root = r == p;
        if (!root) __hip_atomic_store(&lf[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const u64 bal = __ballot(root);
      if (lane == 0 && bal) atomicAdd(&rowcnt[(size_t)f * H + y], __popcll(bal));
    }
  }
}

// one workgroup per frame: rowbase[y] = roots in the rows above y; ncomp = all roots
__global__ void __launch_bounds__(256) k_blob_prefix(int H, const int* __restrict__ rowcnt, int* __restrict__ rowbase, int* __restrict__ ncomp) {
  __shared__ int s_part[256];
  const int t = threadIdx.x, f = blockIdx.x;
  const int per = (H + 255) / 256, lo = min(H, t * per), hi = min(H, lo + per);
  const int* __restrict__ rc = rowcnt + (size_t)f * H;
  int sum = 0;
  for (int y = lo; y < hi; ++y) sum += rc[y];
  s_part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int v = s_part[i]; s_part[i] = run; run += v; }
    ncomp[f] = run;
  }
  __syncthreads();
  int base = s_part[t];
  for (int y = lo; y < hi; ++y) { rowbase[(size_t)f * H + y] = base; base += rc[y]; }
}

// grid (ceil(H / 256), frames): a wave looks at 64 rows, a lane each, and walks those that hold a root; the roots of a row, left
// to right, take the ranks from rowbase[y] on, stored as -(rank + 1) -- a value no index has, so later launches can tell a rank
// from a parent
__global__ void __launch_bounds__(256) k_blob_rank(const BlobParams P, const u64* __restrict__ mask, int* __restrict__ lab,
                                                   const int* __restrict__ rowcnt, const int* __restrict__ rowbase) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const int H = P.height, W = P.width, ww = P.ww;
  const int ywave = (int)blockIdx.x * 256 + (threadIdx.x & ~63);
  u64 rows = __ballot(ywave + lane < H && rowcnt[(size_t)f * H + min(ywave + lane, H - 1)] != 0);
  int* lf = lab + (size_t)f * H * W;
  while (rows) {
    const int y = ywave + __ffsll((long long)rows) - 1;
    rows &= rows - 1;
    const u64* __restrict__ mrow = mask + ((size_t)f * H + y) * ww;
    int run = rowbase[(size_t)f * H + y];
    for (int wb = 0; wb < ww; wb += 64) {
      const u64 ml = wb + lane < ww ? mrow[wb + lane] : 0ull;
      u64 nz = __ballot(ml != 0);
      while (nz) {
        const int j = __ffsll((long long)nz) - 1;
        nz &= nz - 1;
        const u64 m = __shfl(ml, j, 64);
        const int p = y * W + (wb + j) * 64 + lane;
        const bool root = ((m >> lane) & 1) && lf[p] == p;
        const u64 bal = __ballot(root);
        if (root) lf[p] = -(run + __popcll(bal & ((1ull << lane) - 1)) + 1);
        run += __popcll(bal);
      }
    }
  }
}

__device__ __forceinline__ uint32_t blob_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// What a wave has gathered of ONE component over the words it walks; the same in every lane.  Flushed with integer atomics
// when the component changes and at the end: a component that fills the frame costs 12 atomics per BLOB_WAVE_WORDS words.
struct BlobAcc {
  int k;
  u64 s[8];
  int xmin, ymin, xmax, ymax;
};
__device__ __forceinline__ void blob_flush(BlobAcc& A, u64* __restrict__ table, int lane) {
  if (A.k >= 0 && lane == 0) {
    u64* rec = table + (size_t)A.k * BLOB_NREC;
#pragma unroll
    for (int i = 0; i < 8; ++i) if (A.s[i]) atomicAdd(&rec[i], A.s[i]);
    atomicMin(&rec[8], (u64)A.xmin); atomicMin(&rec[9], (u64)A.ymin);
    atomicMax(&rec[10], (u64)A.xmax); atomicMax(&rec[11], (u64)A.ymax);
  }
  A.k = -1;
}

// grid as k_blob_flatten.  Of a word, the pixels of one component are reduced over the wave (the usual word holds one
// component); components beyond max_blobs are numbered but not measured.
__global__ void __launch_bounds__(256) k_blob_stats(const BlobParams P, const u64* __restrict__ raw, const u64* __restrict__ mask,
                                                    const uint8_t* __restrict__ vals, int* __restrict__ lab, u64* __restrict__ table) {
  const int lane = threadIdx.x & 63, f = blockIdx.y;
  const int H = P.height, W = P.width, ww = P.ww;
  const int64_t total = (int64_t)H * ww;
  const int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * BLOB_WAVE_WORDS;
  const u64* __restrict__ mf = mask + (size_t)f * H * ww;
  const u64* __restrict__ rf = raw + (size_t)f * H * ww;
  const uint8_t* __restrict__ vf = vals + (size_t)f * H * W;
  int* lf = lab + (size_t)f * H * W;
  u64* __restrict__ tf = table + (size_t)f * P.max_blobs * BLOB_NREC;
  const uint32_t thr = (uint32_t)P.threshold;
  BlobAcc A;
  A.k = -1;
  for (int64_t base = w0; base < min(total, w0 + BLOB_WAVE_WORDS); base += 64) {
   const u64 ml = base + lane < total ? mf[base + lane] : 0ull;
   const u64 rl = ml ? rf[base + lane] : 0ull;                           // the raw mask lies inside the morphed one
   u64 nz = __ballot(ml != 0);
   while (nz) {
    const int j = __ffsll((long long)nz) - 1;
    nz &= nz - 1;
    const u64 m = __shfl(ml, j, 64), rw = __shfl(rl, j, 64);
    const int64_t s = base + j;
    const int y = (int)(s / ww), wi = (int)(s - (int64_t)y * ww);
    const int x = wi * 64 + lane, p = y * W + x;
    const bool set = (m >> lane) & 1, israw = (rw >> lane) & 1;
    int k = -1;
    if (set) {
      const int v = lf[p];
      k = v < 0 ? -v - 1 : -lf[v] - 1;       // a root holds -(rank + 1); everyone else points at its root (k_blob_flatten)
      if (P.want_labels && v >= 0) lf[p] = -(k + 1);                     // nobody reads the label of a pixel that is no root
    }
    uint32_t w = 0, sat = 0;
    if (israw) { const uint32_t v = vf[p]; w = v - thr; sat = v == 255u; }
    u64 rest = m;
    while (rest) {
      const int leader = __ffsll((long long)rest) - 1;
      const int kk = __shfl(k, leader, 64);
      const bool in = set && k == kk;
      const u64 grp = __ballot(in);
      rest &= ~grp;
      if (kk < 0 || kk >= P.max_blobs) continue;                        // beyond the table: numbered, not measured
      const uint32_t n = __popcll(grp), sx = blob_wave_sum(in ? (uint32_t)x : 0u);
      const uint32_t sw = blob_wave_sum(in ? w : 0u), swx = blob_wave_sum(in ? w * (uint32_t)x : 0u);   // <= 64 * 255 * 16383
      const uint32_t nraw = __popcll(__ballot(in && israw)), nsat = __popcll(__ballot(in && sat));
      const int xlo = wi * 64 + __ffsll((long long)grp) - 1, xhi = wi * 64 + 63 - __clzll((long long)grp);
      if (kk != A.k) {
        blob_flush(A, tf, lane);
        A.k = kk;
#pragma unroll
        for (int i = 0; i < 8; ++i) A.s[i] = 0;
        A.xmin = xlo; A.xmax = xhi; A.ymin = y; A.ymax = y;
      }
      A.s[0] += n; A.s[1] += sx; A.s[2] += (u64)n * (uint32_t)y;
      A.s[3] += nraw; A.s[4] += sw; A.s[5] += swx; A.s[6] += (u64)sw * (uint32_t)y; A.s[7] += nsat;
      A.xmin = min(A.xmin, xlo); A.xmax = max(A.xmax, xhi); A.ymin = min(A.ymin, y); A.ymax = max(A.ymax, y);
    }
   }
  }
  blob_flush(A, tf, lane);
}

// diagnostics: the morphed mask as bytes (into the value plane, which nothing needs any more) and the labels 1, 2, ... in place
// (k_blob_stats has left -(rank + 1) in every pixel of the mask; the rest was never written)
__global__ void __launch_bounds__(256) k_blob_expand(const BlobParams P, const u64* __restrict__ mask, uint8_t* __restrict__ vals,
                                                     int* __restrict__ lab, int want_mask) {
  const int f = blockIdx.y;
  const int H = P.height, W = P.width, ww = P.ww;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const bool set = (mask[((size_t)f * H + y) * ww + (x >> 6)] >> (x & 63)) & 1;
  const size_t p = (size_t)f * H * W + (size_t)i;
  if (want_mask) vals[p] = set ? 1 : 0;
  if (P.want_labels) lab[p] = set ? -lab[p] : 0;
}

// ------------------------------------------------------------------------------------------------ host side
inline void blob_launch(BlobParams P, int channels, int64_t nf, int64_t total_frames, const BlobScratch& S, bool want_mask, hipStream_t st) {
  const int H = P.height, W = P.width, ww = P.ww;
  const int64_t ntab = nf * P.max_blobs * BLOB_NREC;
  hipLaunchKernelGGL(k_blob_init, dim3((unsigned)((ntab + 255) / 256)), dim3(256), 0, st, S.table, ntab);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(S.rowcnt, 0, sizeof(int) * (size_t)nf * H, st));
  {
    const int rpb = P.rows_per_band = frame_rows_per_band(H, total_frames);
    const dim3 grid((unsigned)((H + rpb - 1) / rpb), (unsigned)nf);
    if (channels == 1) hipLaunchKernelGGL(k_blob_threshold<1>, grid, dim3(DOT_THREADS), 0, st, P, S.raw, S.vals);
    else if (channels == 3) hipLaunchKernelGGL(k_blob_threshold<3>, grid, dim3(DOT_THREADS), 0, st, P, S.raw, S.vals);
    else hipLaunchKernelGGL(k_blob_threshold<4>, grid, dim3(DOT_THREADS), 0, st, P, S.raw, S.vals);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_blob_morph, dim3((unsigned)((ww + MORPH_WORDS - 1) / MORPH_WORDS), (unsigned)((H + MORPH_ROWS - 1) / MORPH_ROWS), (unsigned)nf),
                     dim3(MORPH_THREADS), 0, st, P, S.raw, S.mask);
  HIPCHK(hipGetLastError());
  const dim3 tiles((unsigned)((ww + TILE_STRIP - 1) / TILE_STRIP), (unsigned)((H + TILE_ROWS - 1) / TILE_ROWS), (unsigned)nf);
  hipLaunchKernelGGL(k_blob_label_tile, tiles, dim3(TILE_THREADS), 0, st, P, S.mask, S.lab);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_blob_merge, dim3((unsigned)(((int64_t)H * ww + 255) / 256), (unsigned)nf), dim3(256), 0, st, P, S.mask, S.lab);
  HIPCHK(hipGetLastError());
  const dim3 words((unsigned)(((int64_t)H * ww + 4 * BLOB_WAVE_WORDS - 1) / (4 * BLOB_WAVE_WORDS)), (unsigned)nf);
  hipLaunchKernelGGL(k_blob_flatten, words, dim3(256), 0, st, P, S.mask, S.lab, S.rowcnt);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_blob_prefix, dim3((unsigned)nf), dim3(256), 0, st, H, S.rowcnt, S.rowbase, S.ncomp);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_blob_rank, dim3((unsigned)((H + 255) / 256), (unsigned)nf), dim3(256), 0, st, P, S.mask, S.lab, S.rowcnt, S.rowbase);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_blob_stats, words, dim3(256), 0, st, P, S.raw, S.mask, S.vals, S.lab, S.table);
  HIPCHK(hipGetLastError());
  if (want_mask || P.want_labels) {
    hipLaunchKernelGGL(k_blob_expand, dim3((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)nf), dim3(256), 0, st, P, S.mask, S.vals, S.lab,
                       want_mask ? 1 : 0);
    HIPCHK(hipGetLastError());
  }
}

// Acceptance, status and centroid of one frame from its table, on the host (include/sba_hip.h has the rules).  The distance
// test compares (sum x - centre_x n)^2 + (sum y - centre_y n)^2 with (max_centre_dist n)^2 in 128-bit integers: with
// n <= 2^28 and 32-bit centres every term is below 2^60 and every square below 2^120.
inline void blob_judge(const sba_blob_opts& o, int K, int32_t ncomp, uint64_t* rec, int32_t* accepted, double* centroid, int32_t* status) {
  const int listed = std::min<int>(ncomp, K);
  for (int k = listed; k < K; ++k) std::fill(rec + (size_t)k * BLOB_NREC, rec + (size_t)(k + 1) * BLOB_NREC, (uint64_t)0);
  int n_acc = 0, first = -1;
  for (int k = 0; k < listed; ++k) {
    const uint64_t* r = rec + (size_t)k * BLOB_NREC;
    const uint64_t n = r[0];
    bool ok = n >= (uint64_t)o.min_area && (o.max_area == 0 || n <= (uint64_t)o.max_area);
    if (ok && o.max_centre_dist > 0) {
      const __int128 dx = (__int128)r[1] - (__int128)o.centre_x * (__int128)n, dy = (__int128)r[2] - (__int128)o.centre_y * (__int128)n;
      const __int128 lim = (__int128)o.max_centre_dist * (__int128)n;
      ok = dx * dx + dy * dy <= lim * lim;
    }
    if (ok) { if (n_acc == 0) first = k; ++n_acc; }
  }
  const int st = ncomp == 0 ? SBA_BLOB_NONE : ncomp > K ? SBA_BLOB_OVERFLOW : n_acc == 0 ? SBA_BLOB_REJECTED : n_acc > 1 ? SBA_BLOB_MULTIPLE : SBA_BLOB_OK;
  const double nan = std::nan("");
  double c[4] = {nan, nan, nan, nan};
  if (st == SBA_BLOB_OK) {
    const uint64_t* r = rec + (size_t)first * BLOB_NREC;
    c[0] = (double)r[1] / (double)r[0]; c[1] = (double)r[2] / (double)r[0];
    if (r[4]) { c[2] = (double)r[5] / (double)r[4]; c[3] = (double)r[6] / (double)r[4]; }
  }
  if (accepted) *accepted = st == SBA_BLOB_OK ? first : -1;
  if (centroid) std::copy(c, c + 4, centroid);
  if (status) *status = st;
}

// Arguments are checked by the caller (sba_api.hip).  Frames are taken in chunks: of a chunk the scratch above (labels, value
// bytes, the two bit planes: about 5.3 bytes per pixel) stays within BLOB_SCRATCH_BYTES, a single frame always being allowed,
// so device memory does not grow with n_frames.  frames_in_chunks drives them; one set of scratch serves every chunk.
int blob_call(const FrameBatch& B, const sba_blob_opts& o, int32_t* n_components, uint64_t* blobs, int32_t* accepted, double* centroid,
              int32_t* status, uint8_t* mask_out, int32_t* labels_out) {
  const int64_t n_frames = B.n_frames;
  const int32_t height = B.height, width = B.width, channels = B.channels;
  if (n_frames == 0) return SBA_OK;
  const int K = o.max_blobs > 0 ? o.max_blobs : BLOB_DEFAULT_BLOBS;
  std::vector<uint64_t> h_table((size_t)K * BLOB_NREC);
  if (height == 0 || width == 0) {           // no pixel, no component
    for (int64_t f = 0; f < n_frames; ++f) {
      if (n_components) n_components[f] = 0;
      blob_judge(o, K, 0, blobs ? blobs + (size_t)f * K * BLOB_NREC : h_table.data(), accepted ? accepted + f : nullptr,
                 centroid ? centroid + 4 * f : nullptr, status ? status + f : nullptr);
    }
    return SBA_OK;
  }
  HIPCHK(hipSetDevice(B.device));
  BlobParams P{};
  static_cast<FrameView&>(P) = frame_view(B, o.channel, o.threshold, o.roi_rect, o.roi_circle);
  P.ww = (width + 63) / 64;
  P.dh = o.dilate_radius + o.close_radius; P.eh = o.close_radius;
  blob_halfwidths(o.dilate_radius, o.close_radius, P.hwd, P.hwe);
  P.max_blobs = K; P.want_labels = labels_out ? 1 : 0;

  const bool on_device = o.frames_on_device != 0;
  const int64_t px = (int64_t)height * width, words = (int64_t)height * P.ww;
  const int64_t per_frame = px * 5 + words * 16 + (int64_t)height * 8 + (int64_t)K * BLOB_NREC * 8 + 4;
  // neither policy of chunk_of: chunk_frames is a cap here, not a request: the library's own choice, within the scratch budget,
  // bounds it
  int64_t chunk = std::min(frames_per_chunk(0, n_frames, on_device ? 0 : frame_bytes(B)), std::max<int64_t>(1, BLOB_SCRATCH_BYTES / per_frame));
  if (o.chunk_frames > 0) chunk = std::min<int64_t>(chunk, o.chunk_frames);

  DevBuf<uint8_t> d_vals;
  DevBuf<u64> d_raw, d_mask, d_table;
  DevBuf<int> d_lab, d_rowcnt, d_rowbase, d_ncomp;
  d_raw.alloc((size_t)(chunk * words)); d_mask.alloc((size_t)(chunk * words)); d_vals.alloc((size_t)(chunk * px)); d_lab.alloc((size_t)(chunk * px));
  d_rowcnt.alloc((size_t)(chunk * height)); d_rowbase.alloc((size_t)(chunk * height)); d_ncomp.alloc((size_t)chunk);
  d_table.alloc((size_t)chunk * K * BLOB_NREC);
  const BlobScratch S{d_raw.p, d_mask.p, d_vals.p, d_lab.p, d_rowcnt.p, d_rowbase.p, d_ncomp.p, d_table.p};
  std::vector<int32_t> h_ncomp((size_t)chunk);
  if (!blobs) h_table.resize((size_t)chunk * K * BLOB_NREC);

  // where the table of the chunk that starts at frame lo goes
  auto table_of = [&](int64_t lo) { return blobs ? blobs + (size_t)lo * K * BLOB_NREC : h_table.data(); };
  frames_in_chunks(
      P, channels, n_frames, on_device, chunk,
      [&](const FrameView& V, int64_t, int64_t m, hipStream_t st) {
        static_cast<FrameView&>(P) = V;
        blob_launch(P, channels, m, n_frames, S, mask_out != nullptr, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) {
        HIPCHK(hipMemcpyAsync(h_ncomp.data(), d_ncomp.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(table_of(lo), d_table.p, sizeof(uint64_t) * m * K * BLOB_NREC, hipMemcpyDeviceToHost, st));
        if (mask_out) HIPCHK(hipMemcpyAsync(mask_out + lo * px, d_vals.p, (size_t)(m * px), hipMemcpyDeviceToHost, st));
        if (labels_out) HIPCHK(hipMemcpyAsync(labels_out + lo * px, d_lab.p, sizeof(int32_t) * (size_t)(m * px), hipMemcpyDeviceToHost, st));
      },
      [&](int64_t lo, int64_t m) {
        uint64_t* tab = table_of(lo);                // without `blobs`: the host table of this chunk
        for (int64_t i = 0; i < m; ++i) {
          const int64_t f = lo + i;
          if (n_components) n_components[f] = h_ncomp[i];
          blob_judge(o, K, h_ncomp[i], tab + (size_t)i * K * BLOB_NREC, accepted ? accepted + f : nullptr, centroid ? centroid + 4 * f : nullptr,
                     status ? status + f : nullptr);
        }
      });
  return SBA_OK;
}

}  // namespace sba_detect
