// xmaps_k2.hpp -- K2, the frame kernels: 7x7 max (cv2.dilate) composed with the nearest remap (disp_to_depth.py:86-95) -> depth
// (:46-63) -> u8 (:7-21) -> Turbo BGR + white mask (:24-43), on the packed-key frames (64- and 32-bit), on plain f32 / u16
// frames, and the builders of the tables they read (k_build_dlut, k_build_k2_tables).  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp and turbo_lut.inc.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// =====================================================================================================
// K2: frame kernels.
// =====================================================================================================
__device__ const u32 kTurbo[256] = {
#include "turbo_lut.inc"
};

struct PixelOut {
  float depth;
  u32 bgr;  // byte0 = B, byte1 = G, byte2 = R
};

// A5 + A6 + A7 for one pixel of the final disparity frame
__device__ inline PixelOut disparity_pixel(float d, double p03, float z_near, float z_far) {
  PixelOut o;
  // disp_to_depth.py:58-61 -- P2 is float64, so the divide is FP64; max(., 1e-9); stored as f32
  o.depth = d == 0.0f ? 0.0f : (float)fmax(p03 / (double)d, 1e-9);
  // disp_to_depth.py:12-20 -- clamp, normalise in f32; `* 255` is f32 x int64 -> f64 under Numba; trunc
  u32 u8 = 0;
  if (o.depth != 0.0f) {
    const float range = z_far - z_near;
    const float c = fmaxf(fminf(o.depth, z_far), z_near);
    const float q = (c - z_near) / range;
    u8 = (u32)(int)((double)q * 255.0) & 0xff;
  }
  // disp_to_depth.py:24-43 -- Turbo, undefined depth (u8 == 0) painted white
  o.bgr = u8 == 0 ? 0x00ffffffu : kTurbo[u8];
  return o;
}

// The fused path only ever sees integer disparities 0..65535 (low 16 bits of a key), and A5-A7 are a pure function of
// the disparity for fixed P2[0,3] / z_near / z_far: tabulate it once per handle with the very same device function
// (bit-identical by construction) -- K2 then replaces an FP64 divide, an f32 divide and the Turbo lookup by one
// 8-byte gather from a table whose live part (disparities < rect_w) sits in L1/L2.
__global__ __launch_bounds__(BLOCK) void k_build_dlut(uint2* __restrict__ dlut, double p03, float z_near, float z_far) {
  const u32 d = blockIdx.x * BLOCK + threadIdx.x;
  if (d < 65536u) {
    const PixelOut o = disparity_pixel((float)d, p03, z_near, z_far);
    dlut[d] = make_uint2(__float_as_uint(o.depth), o.bgr);
  }
}

// cooperative, coalesced store of BLOCK pixels' BGR bytes (3 B each) through LDS
__device__ inline void store_bgr_block(uint8_t* __restrict__ bgr, u64 first_pixel, u64 n_pixels, u32 v) {
  __shared__ __attribute__((aligned(16))) uint8_t s[BLOCK * 3];
  s[threadIdx.x * 3 + 0] = (uint8_t)(v & 0xff);
  s[threadIdx.x * 3 + 1] = (uint8_t)((v >> 8) & 0xff);
  s[threadIdx.x * 3 + 2] = (uint8_t)((v >> 16) & 0xff);
  __syncthreads();
  const u64 remaining = n_pixels - first_pixel;
  uint8_t* dst = bgr + first_pixel * 3;  // BLOCK*3 = 768 B per block -> 4-byte aligned
  if (remaining >= BLOCK) {
    if (threadIdx.x < BLOCK * 3 / 4) reinterpret_cast<u32*>(dst)[threadIdx.x] = reinterpret_cast<u32*>(s)[threadIdx.x];
  } else {
    for (u32 i = threadIdx.x; i < remaining * 3; i += BLOCK) dst[i] = s[i];
  }
}

struct KeyCells {  // cells of the packed-key frame written by K1 (projector view: column-major)
  static constexpr bool keyed = true;
  const u64* f;
  u32 tag;
  __device__ float decode(u64 k) const { return (u32)(k >> KEY_TAG_SHIFT) == tag ? (float)(u32)(k & 0xffff) : 0.0f; }
  __device__ float get(u32 i) const { return decode(f[i]); }
  __device__ float at(const DevTables& tb, int col, int row) const { return decode(f[(u32)col * (u32)tb.rect_h + (u32)row]); }
};
struct F32Cells {  // a plain row-major f32 disparity frame (stage API)
  static constexpr bool keyed = false;
  const float* f;
  __device__ float get(u32 i) const { return f[i]; }
  __device__ float at(const DevTables& tb, int col, int row) const { return f[(u32)row * (u32)tb.rect_w + (u32)col]; }
};

// dilate(7x7) o remap(nearest) composed: out[v,u] = max over the 7x7 window centred on map[v,u] of the
// rectified frame, 0 when the map points outside it; window cells outside the image are ignored.
template <typename Cells>
__device__ inline float dilated_remap(const Cells& cells, const DevTables& tb, u32 pixel) {
  const u32 m = tb.pmap[pixel];
  const int mx = (int)(short)(m & 0xffff), my = (int)(short)(m >> 16);
  if (mx < 0 || mx >= tb.rect_w || my < 0 || my >= tb.rect_h) return 0.0f;  // BORDER_CONSTANT 0
  float best = 0.0f;  // disparities are >= 0, so ignoring the border == zero padding
  const int y0 = max(my - 3, 0), y1 = min(my + 3, tb.rect_h - 1);
  const int x0 = max(mx - 3, 0), x1 = min(mx + 3, tb.rect_w - 1);
  for (int xx = x0; xx <= x1; ++xx) {
#pragma unroll 7
    for (int yy = y0; yy <= y1; ++yy) best = fmaxf(best, cells.at(tb, xx, yy));
  }
  return best;
}

// projector view: one thread per projector pixel.  MODE 0: packed-key frame -> depth + BGR (fused hot
// path); MODE 1: f32 frame -> f32 remapped disparity (stage A4)
template <typename Cells, int MODE>
__global__ __launch_bounds__(BLOCK) void k_frame_proj(Cells cells, DevTables tb, SlotState* st, u32 tag_override,
                                                      float* __restrict__ out_f32, uint8_t* __restrict__ bgr) {
  const u64 n_pixels = (u64)tb.proj_w * tb.proj_h;
  const u64 pixel = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if constexpr (MODE == 0) {
    const u32 tag = tag_override ? tag_override : st->tag_a;
    cells.tag = tag;
    if (!tag_override && blockIdx.x == 0 && threadIdx.x < CNT_SLOTS) {  // re-arm the next frame's counters
      u32* c = st->cnt[(tag & 1) ^ 1][threadIdx.x];
      c[0] = c[1] = c[2] = c[3] = 0;
      if (threadIdx.x == 0) {
        st->tag_b = tag;
        if (u32* hf = st->host_flags) host_flag_store(hf + 1, tag);
      }
    }
  }
  float d = 0.0f;
  if (pixel < n_pixels) d = dilated_remap(cells, tb, (u32)pixel);
  if constexpr (MODE == 1) {
    if (pixel < n_pixels) out_f32[pixel] = d;
  } else {
    const PixelOut o = disparity_pixel(d, tb.p03, tb.z_near, tb.z_far);
    if (out_f32 && pixel < n_pixels) out_f32[pixel] = o.depth;
    if (bgr) store_bgr_block(bgr, (u64)blockIdx.x * BLOCK, n_pixels, o.bgr);
  }
}


// K2 (tiled, projector view, fused path): one block of 16 x 16 threads = a 32 x 16 tile of projector pixels, two per thread
// (K2_PPT: a K2 wave is a chain of dependent round trips -- descriptor, tile record, patch, table -- and what it costs is
// resident waves x lifetime, so each wave carries two pixels' worth of loads through that chain; measured against 1, 3, 4
// pixels per thread and 64x8 / 16x32 tiles: DESIGN.md section 3).  Their map targets span a (32*sx+6) x (16*sy+6) patch of
// the rectified key frame (sx, sy ~ 2.75):
//   0. the patch rectangle of the tile and every pixel's offset into it are static (the maps never change): they come
//      from tables built once in xm_create (k_build_k2_tables), so the loads below start right after one uniform load;
//   1. the patch is loaded ONCE into LDS as u16 disparities (stale tags -> 0, cells outside the frame -> 0); the key
//      frame is column-major, so the patch is `cols` contiguous runs -> paired 16-byte loads, 8 in flight per thread;
//   2. the 7-tap max along rows is taken once per patch cell with 16-byte LDS reads (separable max filter);
//   3. every pixel then needs 7 LDS reads (one per window column) instead of 49.
// PMC on the 49-tap version: SQ_LDS_IDX_ACTIVE 3.1 M cycles / dispatch -- it was LDS-bound.
// Falls back to global reads when the patch does not fit (wild maps).
#ifdef XM_ABLATE  // experiments (tools/k2_timeline.py): s_memtime stamps of thread 0 of 64 tiles in the middle of frame 30's K2
#define XM_K2STAMP(ph) do { if (threadIdx.x == 0 && blockIdx.z == 30 && blockIdx.y == 15 && blockIdx.x < 40) g_timeline[blockIdx.x][9 + (ph)] = __builtin_amdgcn_s_memtime(); } while (0)  /* columns 9..15: K1's stamps keep 0..8 */
#else
#define XM_K2STAMP(ph) do { } while (0)
#endif
// pixels per thread (template parameter PPT of the K2 kernels: 2 for launches that fill the chip, 1 for a lone frame): a block's
// tile is K2_TX * PPT x K2_TY pixels, thread (tx, ty) takes columns tx + j * K2_TX  (K2_TX, K2_TY, K2_TILE_MAX: xmaps_geometry.hpp)

__device__ inline uint16_t key_disp(u64 k, u32 tag) { return (u32)(k >> KEY_TAG_SHIFT) == tag ? (uint16_t)(k & 0xffff) : (uint16_t)0; }

// One-off (xm_create): per K2 tile, the bounding box of its pixels' map targets (+3 cells of dilate margin, rows starting
// on an even row and padded to 8) and, per pixel, where its window starts inside that patch.  The maps are static, so
// K2 no longer decodes the map, reduces a bounding box over the block and synchronises before it can issue its loads.
template <int PPT>
__global__ __launch_bounds__(K2_TX* K2_TY) void k_build_k2_tables(DevTables tb, int4* __restrict__ tiles,
                                                                 u32* __restrict__ pix) {
  constexpr int K2_PPT = PPT, K2_TW = K2_TX * PPT;
  constexpr int NT = K2_TX * K2_TY, NW = NT / 64;
  __shared__ int s_box[NW][4];
  const int tid = threadIdx.x, tx = tid % K2_TX, ty = tid / K2_TX;
  const int v = blockIdx.y * K2_TY + ty;
  int u[K2_PPT], mx[K2_PPT], my[K2_PPT];
  bool in_img[K2_PPT], valid[K2_PPT];
  int x0 = 0x7fffffff, x1 = -0x7fffffff, y0 = 0x7fffffff, y1 = -0x7fffffff;
#pragma unroll
  for (int j = 0; j < K2_PPT; ++j) {
    u[j] = blockIdx.x * K2_TW + tx + j * K2_TX;
    in_img[j] = u[j] < tb.proj_w && v < tb.proj_h;
    mx[j] = my[j] = 0;
    valid[j] = false;
    if (in_img[j]) {
      const u32 m = tb.pmap[(u32)v * (u32)tb.proj_w + (u32)u[j]];
      mx[j] = (int)(short)(m & 0xffff);
      my[j] = (int)(short)(m >> 16);
      valid[j] = mx[j] >= 0 && mx[j] < tb.rect_w && my[j] >= 0 && my[j] < tb.rect_h;
    }
    if (valid[j]) {
      x0 = min(x0, mx[j]);
      x1 = max(x1, mx[j]);
      y0 = min(y0, my[j]);
      y1 = max(y1, my[j]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o, 64));
    x1 = max(x1, __shfl_xor(x1, o, 64));
    y0 = min(y0, __shfl_xor(y0, o, 64));
    y1 = max(y1, __shfl_xor(y1, o, 64));
  }
  if ((tid & 63) == 0) {
    s_box[tid >> 6][0] = x0;
    s_box[tid >> 6][1] = x1;
    s_box[tid >> 6][2] = y0;
    s_box[tid >> 6][3] = y1;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    x0 = min(x0, s_box[w][0]);
    x1 = max(x1, s_box[w][1]);
    y0 = min(y0, s_box[w][2]);
    y1 = max(y1, s_box[w][3]);
  }
  int4 rec = make_int4(0, 0, 0, 0);
  u32 off[K2_PPT];
#pragma unroll
  for (int j = 0; j < K2_PPT; ++j) off[j] = ~0u;
  if (x1 >= x0) {
    // rows start on a multiple of 8: 16-byte loads of 2 (u64 keys), 4 (u32 keys) or 8 (u16 disparities) rows
    const int bx = x0 - 3, by = (y0 - 3) & ~7;
    const int cols = x1 + 3 - bx + 1, rows = y1 + 3 - by + 1, rows_p = (rows + 7) & ~7;
    const bool fits = cols * rows_p <= K2_TILE_MAX;
    rec = make_int4(bx, by, fits ? cols : -1, rows_p);
#pragma unroll
    for (int j = 0; j < K2_PPT; ++j)
      if (valid[j] && fits) off[j] = (u32)((mx[j] - 3 - bx) * rows_p + (my[j] - 3 - by));
  }
  if (tid == 0) tiles[blockIdx.y * gridDim.x + blockIdx.x] = rec;
#pragma unroll
  for (int j = 0; j < K2_PPT; ++j)
    if (in_img[j]) pix[(u32)v * (u32)tb.proj_w + (u32)u[j]] = off[j];
}

// 7-tap max along 8 consecutive rows of a patch column: inputs e[0..13] = the 16 bytes a (rows r .. r+7) and b (rows r+8 .. r+15),
// outputs o[j] = max(e[j] .. e[j+6]), j = 0..7.  Packed 16-bit arithmetic (v_pk_max_u16): P_k = (e[2k], e[2k+1]) as loaded,
// S_k = (e[2k+1], e[2k+2]) by a 16-bit funnel shift; (o[2j], o[2j+1]) = max(P_j, S_j, P_j+1, S_j+1, P_j+2, S_j+2, P_j+3):
// 24 instructions instead of 72 for unpack + 48 scalar maxima + pack
__device__ __forceinline__ uint4 k2_rowmax8(const uint4 a, const uint4 b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const auto pk = [](u32 v) { u16x2 r; __builtin_memcpy(&r, &v, 4); return r; };
  const auto up = [](u16x2 v) { u32 r; __builtin_memcpy(&r, &v, 4); return r; };
  const auto mx = [](u16x2 x, u16x2 y) { return __builtin_elementwise_max(x, y); };
  const u32 P[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
  u16x2 M[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) M[k] = mx(pk(P[k]), pk(__builtin_amdgcn_alignbit(P[k + 1], P[k], 16)));
  uint4 w;
  w.x = up(mx(mx(M[0], M[1]), mx(M[2], pk(P[3]))));
  w.y = up(mx(mx(M[1], M[2]), mx(M[3], pk(P[4]))));
  w.z = up(mx(mx(M[2], M[3]), mx(M[4], pk(P[5]))));
  w.w = up(mx(mx(M[3], M[4]), mx(M[5], pk(P[6]))));
  return w;
}

// ---- Pieces of a K2 block written once.  Only those whose extraction left every kernel's assembly byte for byte as it was are
// here; the stages that did not (row maxima, 7-tap sample, output writer, the patch loaders) stay spelled out at their sites:
// profiles/k2_stages_identity.md has the table.

// (i / n, i % n) without the integer divide: the quotient through inv_n ~ 1 / n in float (approximate is enough: the +-1 fix-ups
// absorb it).  MUL24: q * n by the full-rate 24-bit multiply.  (By value: through references such a helper moved assembly)
struct K2DivMod {
  int q, r;
};
template <bool MUL24 = false>
__device__ __forceinline__ K2DivMod k2_divmod(int i, int n, float inv_n) {
  int q = (int)((float)i * inv_n), r = i - (MUL24 ? __mul24(q, n) : q * n);
  if (r < 0) { q -= 1; r += n; }
  if (r >= n) { q += 1; r -= n; }
  return {q, r};
}

// Re-arm the next frame's counters (threads tid < CNT_SLOTS of the frame's first tile) and publish the tag: frame_proj_tiled_body
// and k_frame_proj_pipe (xmaps_k2pipe.hpp).  State: SlotState*, or the pipelined kernel's pointer into the global address space
template <typename State>
__device__ __forceinline__ void k2_rearm_counters(State st, u32 tag, int tid) {
  auto* c = st->cnt[(tag & 1) ^ 1][tid];
  c[0] = c[1] = c[2] = c[3] = 0;
  if (tid == 0) {
    st->tag_b = tag;  // time-sorted mode: K1 derived the tag from tag_b without touching it
    if (u32* hf = st->host_flags) host_flag_store(hf + 1, tag);
  }
}

// blk_lin / grid_x / grid_y = linear block index inside the frame's tile grid and that grid's shape
// FMT: what `keys` points at -- 0: the 64-bit packed-key frame; 1: the compact 32-bit key frame of the verified-sorted path
// (see key32_tag); 2: a plain u16 disparity frame, no tags (sharded frames after reduce-scatter + all-gather, xm_shard_finish_u16)
template <int FMT = 0, int PPT = 2>
__device__ __forceinline__ void frame_proj_tiled_body(const u64* __restrict__ keys, const DevTables& tb, SlotState* st,
                                                      u32 tag_override, const unsigned char* __restrict__ dirty,
                                                      const ulonglong2* __restrict__ zero16, float* __restrict__ depth,
                                                      uint8_t* __restrict__ bgr, int tile_cap, const u32 blk_lin,
                                                      const u32 grid_x, const u32 grid_y, const int4* rec_pre = nullptr) {
  // Dynamic LDS sized to the largest patch of THIS rig (tile_cap cells, a multiple of 8, <= K2_TILE_MAX; set in xm_create):
  // how many blocks fit beside K1's 70 KB blocks on a CU is what bounds the pipelined frame rate, and the static
  // worst case was several times what C-1M's 94 x 56 patches need.
  constexpr bool KEY32 = FMT == 1, U16 = FMT == 2;
  constexpr int K2_PPT = PPT, K2_TW = K2_TX * PPT;
  extern __shared__ __attribute__((aligned(16))) uint16_t k2_lds[];
  uint16_t* tile = k2_lds;  // [k2_patch_hw(tile_cap)]: the patch and the overrun of its last 16-byte reads
  uint16_t* vmax = tile;  // the row maxima replace the patch IN PLACE: half the LDS per block = more blocks per CU
  constexpr int NT = K2_TX * K2_TY, NW = NT / 64;
  __shared__ __attribute__((aligned(16))) uint8_t s_bgr[K2_TY][K2_TW * 3];
  constexpr int FLAG_LINES = 8, FLAG_COLS = 128;  // patch columns x 128-byte lines per column (rows_p <= 96 -> <= 7 lines)
  __shared__ unsigned char s_live[FLAG_COLS * FLAG_LINES];
  const int tid = threadIdx.x, tx = tid & (K2_TX - 1), ty = tid / K2_TX;
  XM_K2STAMP(0);
  // XCD-aware tile order (see xcd_contiguous): each XCD takes a contiguous run of the tile raster, so the halos that
  // neighbouring tiles share (3 of 22 patch columns each side, boundary cache lines above/below) hit in its own L2.
  const u32 lin_tile = xcd_contiguous(blk_lin, grid_x * grid_y);
  const u32 tile_y = lin_tile / grid_x, tile_x = lin_tile - tile_y * grid_x;
  const u32 tag = tag_override ? tag_override : st->tag_a;  // first needed when the patch is decoded
  const int v = tile_y * K2_TY + ty;
  // the tile's patch rectangle and the pixel's offset into it were computed once in xm_create (k_build_k2_tables)
  const int4 rec = rec_pre ? *rec_pre : (PPT == 1 ? tb.k2_tiles1 : tb.k2_tiles)[lin_tile];  // block-uniform
  const u32* __restrict__ k2_pix = PPT == 1 ? tb.k2_pix1 : tb.k2_pix;
  bool in_img[K2_PPT];
  u32 pix_i[K2_PPT], poff[K2_PPT];
#pragma unroll
  for (int j = 0; j < K2_PPT; ++j) {
    const int u = tile_x * K2_TW + tx + j * K2_TX;
    in_img[j] = u < tb.proj_w && v < tb.proj_h;
    pix_i[j] = __umul24((u32)v, (u32)tb.proj_w) + (u32)u;  // (24-bit multiplies are full rate, v_mul_lo_u32 a quarter)
    poff[j] = in_img[j] ? k2_pix[pix_i[j]] : ~0u;
  }
  // (poff is tested where it is needed, after the patch loads are out: testing it here put a full wait for this load in
  // front of them)
  float d[K2_PPT];  // generic path (a patch too large for LDS)
  u32 di[K2_PPT];   // tiled path: the integer disparity itself (no int -> float -> int round trip: conversions are quarter rate)
#pragma unroll
  for (int j = 0; j < K2_PPT; ++j) {
    d[j] = 0.0f;
    di[j] = 0;
  }
  if (rec.z != 0) {  // at least one pixel of the tile maps into the frame (rec.z < 0: into a patch too large for LDS)
    const int bx = rec.x, by = rec.y;                    // patch origin (rows start on an even row: 16-byte aligned pairs)
    const int cols = rec.z, rows_p = rec.w;              // column stride in LDS: 16-byte aligned runs
    if (cols > 0) {
      constexpr int UN = 8;
      // which 128-byte lines of the patch carry keys of THIS frame?  (flag bytes written by K1; all lines when no flags)
      const bool use_flags = dirty != nullptr && cols <= FLAG_COLS && rows_p <= 16 * (FLAG_LINES - 1);
      if (use_flags) {
        const unsigned char want = dirty_byte(tag);
        const u32 n_lines = ((u32)tb.rect_w * (u32)tb.rect_h + 15u) >> 4;
        for (int i = tid; i < cols * FLAG_LINES; i += NT) {
          const int c = i / FLAG_LINES, j = i - c * FLAG_LINES, gx = bx + c;
          unsigned char live = 0;
          if (gx >= 0 && gx < tb.rect_w) {
            const int first_cell = gx * tb.rect_h + max(by, 0);  // first in-frame cell of this patch column
            const u32 line = ((u32)first_cell >> 4) + (u32)j;
            if (line < n_lines) live = dirty[line] == want;
          }
          s_live[i] = live;
        }
        __syncthreads();
      }
      if constexpr (U16) {  // plain disparities: 8-byte loads of 4 rows copied straight into the LDS patch
        const uint16_t* d16 = reinterpret_cast<const uint16_t*>(keys);
        const bool interior = bx >= 0 && by >= 0 && bx + cols <= tb.rect_w && by + rows_p <= tb.rect_h && (tb.rect_h & 3) == 0;
        const int g0 = by >> 3, sh0 = tb.shear_bias + ((g0 * tb.shear_m) >> 12);  // the patch's first 8-row group and its shear
        if (interior && (tb.rect_h & 7) == 0) {
          // 16-byte loads of 8 rows (the patch starts on a multiple of 8 rows and rows_p is one), copied as they are: LDS quad
          // index == patch (column, row octet) index.  A 50 x 56 patch is 350 quads: two loads per thread.
          const int oct = rows_p >> 3, total = cols * oct;
          if (oct <= 8) {
            // patches of <= 64 rows: thread slot s -> (column s >> 3, row octet s & 7) by shift and mask (slots with an octet
            // past the patch idle); K2 is issue bound and the divide by `oct` below is ~12 instructions per load
            const int nslot = cols << 3;
            for (int s0 = tid; s0 < nslot; s0 += 2 * NT) {
              uint4 k[2];
              bool has[2];
#pragma unroll
              for (int j = 0; j < 2; ++j) {
                const int sj = s0 + j * NT, c = sj >> 3, ro = sj & 7;
                has[j] = sj < nslot && ro < oct;
                // (the frame is sheared by whole columns per 8-row group -- frame16_col; sh0 / shear_m are 0 on rigs that are not slanted)
                const int cs = bx + c + (((g0 + ro) * tb.shear_m) >> 12);
                k[j] = *reinterpret_cast<const uint4*>(d16 + (has[j] ? __umul24((u32)(cs + tb.shear_bias), (u32)tb.rect_h) + (u32)(by + 8 * ro)
                                                                     : __umul24((u32)(bx + sh0), (u32)tb.rect_h) + (u32)by));
              }
#pragma unroll
              for (int j = 0; j < 2; ++j) {
                const int sj = s0 + j * NT;
                if (has[j]) reinterpret_cast<uint4*>(tile)[__mul24(sj >> 3, oct) + (sj & 7)] = k[j];
              }
            }
          } else {
          const float inv_o = __builtin_amdgcn_rcpf((float)oct);  // (approximate: k2_divmod's +-1 fix-ups absorb it)
          for (int i0 = tid; i0 < total; i0 += 2 * NT) {
            uint4 k[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const K2DivMod at = k2_divmod<true>(min(i0 + j * NT, total - 1), oct, inv_o);
              const int c = at.q, ro = at.r;
              k[j] = *reinterpret_cast<const uint4*>(d16 + __umul24((u32)(bx + c + tb.shear_bias + (((g0 + ro) * tb.shear_m) >> 12)), (u32)tb.rect_h) +
                                                     (u32)(by + 8 * ro));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
              if (i0 + j * NT < total) reinterpret_cast<uint4*>(tile)[i0 + j * NT] = k[j];
          }
          }
        } else if (interior) {
          const int quarter = rows_p >> 2, total = cols * quarter;
          const float inv_q = __builtin_amdgcn_rcpf((float)quarter);
          for (int i0 = tid; i0 < total; i0 += 4 * NT) {
            uint2 k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const K2DivMod at = k2_divmod<true>(min(i0 + j * NT, total - 1), quarter, inv_q);
              const int c = at.q, rq = at.r;
              k[j] = *reinterpret_cast<const uint2*>(d16 + __umul24((u32)frame16_col(tb, bx + c, by + 4 * rq), (u32)tb.rect_h) + (u32)(by + 4 * rq));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (i0 + j * NT < total) reinterpret_cast<uint2*>(tile)[i0 + j * NT] = k[j];
          }
        } else {
          const int total = cols * rows_p;
          const float inv_rows = 1.0f / (float)rows_p;
          for (int i = tid; i < total; i += NT) {
            int c = (int)((float)i * inv_rows), r = i - c * rows_p;
            if (r < 0) { c -= 1; r += rows_p; }
            if (r >= rows_p) { c += 1; r -= rows_p; }
            const int gx = bx + c, gy = by + r;
            const bool inside = gx >= 0 && gx < tb.rect_w && gy >= 0 && gy < tb.rect_h;
            const int cx = min(max(gx, 0), tb.rect_w - 1), cy = min(max(gy, 0), tb.rect_h - 1);
            const uint16_t v = d16[(u32)frame16_col(tb, cx, cy) * (u32)tb.rect_h + (u32)cy];
            tile[i] = inside ? v : (uint16_t)0;
          }
        }
      } else if constexpr (KEY32) {
        const u32* keys32 = reinterpret_cast<const u32*>(keys);
        const u32 tag4 = key32_tag(tag);
        const bool interior = bx >= 0 && by >= 0 && bx + cols <= tb.rect_w && by + rows_p <= tb.rect_h;  // rect_h % 4 == 0 (host)
        if (interior) {  // 16-byte loads of 4 consecutive rows, (column, row quad) advanced incrementally
          const int quarter = rows_p >> 2, total = cols * quarter;
          const int dq = NT / quarter, dr = NT - dq * quarter;
          int c_i = (int)((float)tid * (1.0f / (float)quarter)), rq_i = tid - c_i * quarter;
          if (rq_i < 0) { c_i -= 1; rq_i += quarter; }
          if (rq_i >= quarter) { c_i += 1; rq_i -= quarter; }
          u32 cell = (u32)(bx + c_i) * (u32)tb.rect_h + (u32)(by + 4 * rq_i);
          const u32 cell_origin = (u32)bx * (u32)tb.rect_h + (u32)by;
          const u32 dcell = (u32)dq * (u32)tb.rect_h + 4u * (u32)dr, carry = (u32)tb.rect_h - 4u * (u32)quarter;
          auto pass = [&](auto un_tag) {
            constexpr int UL = decltype(un_tag)::value;
            for (int i0 = tid; i0 < total; i0 += UL * NT) {
              uint4 k[UL];
#pragma unroll
              for (int j = 0; j < UL; ++j) {
                k[j] = *reinterpret_cast<const uint4*>(keys32 + (i0 + j * NT < total ? cell : cell_origin));
                cell += dcell;
                rq_i += dr;
                if (rq_i >= quarter) { rq_i -= quarter; cell += carry; }
              }
#pragma unroll
              for (int j = 0; j < UL; ++j) {
                const int i = i0 + j * NT;
                if (i < total)
                  reinterpret_cast<uint2*>(tile)[i] =
                      make_uint2((u32)key_disp32(k[j].x, tag4) | ((u32)key_disp32(k[j].y, tag4) << 16),
                                 (u32)key_disp32(k[j].z, tag4) | ((u32)key_disp32(k[j].w, tag4) << 16));
              }
            }
          };
          const int need = (total + NT - 1) / NT;
          if (need <= 1) pass(std::integral_constant<int, 1>{});
          else if (need <= 2) pass(std::integral_constant<int, 2>{});
          else if (need <= 3) pass(std::integral_constant<int, 3>{});
          else pass(std::integral_constant<int, 4>{});
        } else {  // patches that stick out of the frame (tiles along the border): cell by cell
          const int total = cols * rows_p;
          const float inv_rows = 1.0f / (float)rows_p;
          for (int i = tid; i < total; i += NT) {
            int c = (int)((float)i * inv_rows), r = i - c * rows_p;
            if (r < 0) { c -= 1; r += rows_p; }
            if (r >= rows_p) { c += 1; r -= rows_p; }
            const int gx = bx + c, gy = by + r;
            const bool inside = gx >= 0 && gx < tb.rect_w && gy >= 0 && gy < tb.rect_h;
            const u32 kk = keys32[(u32)min(max(gx, 0), tb.rect_w - 1) * (u32)tb.rect_h + (u32)min(max(gy, 0), tb.rect_h - 1)];
            tile[i] = inside ? key_disp32(kk, tag4) : (uint16_t)0;
          }
        }
      } else if ((tb.rect_h & 1) == 0) {
        const int half = rows_p >> 1, total = cols * half;
        // (c, rp) = divmod(i, half) advanced incrementally: i -> i + NT is (c + dq, rp + dr) with one carry
        const int dq = NT / half, dr = NT - dq * half;
        int c_i = (int)((float)tid * (1.0f / (float)half)), rp_i = tid - c_i * half;  // no integer divide
        if (rp_i < 0) { c_i -= 1; rp_i += half; }
        if (rp_i >= half) { c_i += 1; rp_i -= half; }
        // K2 is bound by instruction issue, and most tiles' patches lie entirely inside the frame: those take a lean
        // loader -- the cell index advances incrementally with the (column, row pair) carry, no clamps, no inside tests --
        // unrolled to what the patch needs (a 46 x 24 patch is 2.2 sixteen-byte loads per thread, not 8).
        const bool interior = !use_flags && bx >= 0 && by >= 0 && bx + cols <= tb.rect_w && by + rows_p <= tb.rect_h;
        if (interior) {
          u32 cell = (u32)(bx + c_i) * (u32)tb.rect_h + (u32)(by + 2 * rp_i);
          const u32 cell_origin = (u32)bx * (u32)tb.rect_h + (u32)by;
          const u32 dcell = (u32)dq * (u32)tb.rect_h + 2u * (u32)dr, carry = (u32)tb.rect_h - 2u * (u32)half;
          auto pass = [&](auto un_tag) {
            constexpr int UL = decltype(un_tag)::value;
            for (int i0 = tid; i0 < total; i0 += UL * NT) {
              ulonglong2 k[UL];
#pragma unroll
              for (int j = 0; j < UL; ++j) {
                k[j] = *reinterpret_cast<const ulonglong2*>(keys + (i0 + j * NT < total ? cell : cell_origin));
                cell += dcell;
                rp_i += dr;
                if (rp_i >= half) { rp_i -= half; cell += carry; }
              }
#pragma unroll
              for (int j = 0; j < UL; ++j) {
                const int i = i0 + j * NT;
                if (i < total)
                  reinterpret_cast<u32*>(tile)[i] = (u32)key_disp(k[j].x, tag) | ((u32)key_disp(k[j].y, tag) << 16);
              }
            }
          };
          const int need = (total + NT - 1) / NT;
          if (need <= 2) pass(std::integral_constant<int, 2>{});
          else if (need <= 3) pass(std::integral_constant<int, 3>{});
          else if (need <= 4) pass(std::integral_constant<int, 4>{});
          else pass(std::integral_constant<int, 8>{});
        } else
        for (int i0 = tid; i0 < total; i0 += UN * NT) {
          ulonglong2 k[UN];
          bool inside[UN];
#pragma unroll
          for (int j = 0; j < UN; ++j) {  // unconditional loads (coordinates clamped into the frame), select afterwards
            const int gx = bx + c_i, gy = by + 2 * rp_i;
            inside[j] = gx >= 0 && gx < tb.rect_w && gy >= 0 && gy < tb.rect_h;
            const int cx = min(max(gx, 0), tb.rect_w - 1), cy = min(max(gy, 0), tb.rect_h - 2);
            const u32 cell = (u32)cx * (u32)tb.rect_h + (u32)cy;
            const ulonglong2* src = reinterpret_cast<const ulonglong2*>(keys + cell);
            if (use_flags) {  // clean line: read the 16-byte zero constant instead (L2-hot, no HBM traffic)
              const int first_cell = cx * tb.rect_h + max(by, 0);
              const int jl = (int)(cell >> 4) - (first_cell >> 4);
              const bool live = inside[j] && (u32)jl < (u32)FLAG_LINES && s_live[min(c_i, FLAG_COLS - 1) * FLAG_LINES + max(min(jl, FLAG_LINES - 1), 0)];
              inside[j] = live;
              src = live ? src : zero16;
            }
            k[j] = *src;
            c_i += dq;
            rp_i += dr;
            if (rp_i >= half) { rp_i -= half; c_i += 1; }
          }
#pragma unroll
          for (int j = 0; j < UN; ++j) {
            const int i = i0 + j * NT;
            if (i < total) {
              const u32 pr = inside[j] ? ((u32)key_disp(k[j].x, tag) | ((u32)key_disp(k[j].y, tag) << 16)) : 0u;
              reinterpret_cast<u32*>(tile)[i] = pr;  // tile[c * rows_p + 2 * rp] (+1): i == c * half + rp
            }
          }
        }
      } else {
        const int total = cols * rows_p;
        const float inv_rows = 1.0f / (float)rows_p;
        for (int i0 = tid; i0 < total; i0 += UN * NT) {
          u64 k[UN];
          bool inside[UN];
#pragma unroll
          for (int j = 0; j < UN; ++j) {
            const K2DivMod at = k2_divmod(min(i0 + j * NT, total - 1), rows_p, inv_rows);
            const int gx = bx + at.q, gy = by + at.r;
            inside[j] = gx >= 0 && gx < tb.rect_w && gy >= 0 && gy < tb.rect_h;
            const int cx = min(max(gx, 0), tb.rect_w - 1), cy = min(max(gy, 0), tb.rect_h - 1);
            k[j] = keys[(u32)cx * (u32)tb.rect_h + (u32)cy];
          }
#pragma unroll
          for (int j = 0; j < UN; ++j) {
            const int i = i0 + j * NT;
            if (i < total) tile[i] = inside[j] ? key_disp(k[j], tag) : (uint16_t)0;
          }
        }
      }
      XM_K2STAMP(1);
      __syncthreads();
      XM_K2STAMP(2);
      {  // 7-tap max along the rows of every patch column: 8 outputs per task from 14 inputs (two 16-byte LDS reads).
        // (Tried: taking them in registers straight from two global loads per thread, no tile buffer and one barrier less --
        // the kernel alone is as fast, the pipelined frame rate 4 % lower: twice the vector-memory requests.)
        // Task t covers tile[t*8 .. t*8+7] (c*rows_p + 8*seg) and reads 6 cells of task t + 1.  In place: a chunk of 4 NT
        // consecutive tasks is computed into registers, a barrier, then stored over its own inputs; the next chunk's inputs
        // lie behind everything this one wrote.
        const int nseg = rows_p >> 3, tasks = cols * nseg;
        constexpr int CH = 4;
        for (int t0 = 0; t0 < tasks; t0 += CH * NT) {  // (block-uniform trip count)
          uint4 w[CH];
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const int t = t0 + j * NT + tid;
            if (t < tasks)
              w[j] = k2_rowmax8(*reinterpret_cast<const uint4*>(tile + t * 8), *reinterpret_cast<const uint4*>(tile + t * 8 + 8));
          }
          __syncthreads();
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const int t = t0 + j * NT + tid;
            if (t < tasks) *reinterpret_cast<uint4*>(vmax + t * 8) = w[j];
          }
        }
      }
      XM_K2STAMP(3);
      __syncthreads();
      XM_K2STAMP(4);
#pragma unroll
      for (int q = 0; q < K2_PPT; ++q)
        if (poff[q] != ~0u) {
          const uint16_t* p = vmax + poff[q];
          u32 best = 0;
#pragma unroll
          for (int j = 0; j < 7; ++j) best = max(best, (u32)p[j * rows_p]);
          di[q] = best;
        }
    } else {
      for (int q = 0; q < K2_PPT; ++q) {
        if (!in_img[q]) continue;
        const u32 m = tb.pmap[pix_i[q]];
        const int mx = (int)(short)(m & 0xffff), my = (int)(short)(m >> 16);
        if (!(mx >= 0 && mx < tb.rect_w && my >= 0 && my < tb.rect_h)) continue;  // BORDER_CONSTANT 0
        const int ya = max(my - 3, 0), yb = min(my + 3, tb.rect_h - 1), xa = max(mx - 3, 0), xb = min(mx + 3, tb.rect_w - 1);
        float dq = 0.0f;
        if constexpr (U16) {
          const uint16_t* d16 = reinterpret_cast<const uint16_t*>(keys);
          for (int xx = xa; xx <= xb; ++xx)
            for (int yy = ya; yy <= yb; ++yy) dq = fmaxf(dq, (float)d16[(u32)frame16_col(tb, xx, yy) * (u32)tb.rect_h + (u32)yy]);
        } else if constexpr (KEY32) {
          const u32* keys32 = reinterpret_cast<const u32*>(keys);
          const u32 tag4 = key32_tag(tag);
          for (int xx = xa; xx <= xb; ++xx)
            for (int yy = ya; yy <= yb; ++yy) dq = fmaxf(dq, (float)key_disp32(keys32[(u32)xx * (u32)tb.rect_h + (u32)yy], tag4));
        } else {
          KeyCells cells{keys, tag};
          for (int xx = xa; xx <= xb; ++xx)
            for (int yy = ya; yy <= yb; ++yy) dq = fmaxf(dq, cells.at(tb, xx, yy));
        }
        d[q] = dq;
      }
    }
  }
  XM_K2STAMP(5);
  PixelOut o[K2_PPT];
#pragma unroll
  for (int q = 0; q < K2_PPT; ++q) {
    if (rec.z <= 0) di[q] = (u32)d[q];  // d is an integer disparity here (max of u16 key fields)
    // (byte offset off the table's base: a scalar-base + 32-bit-offset load instead of a 64-bit multiply-add per pixel)
    const uint2 e = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(tb.dlut) + ((di[q] & 0xffffu) << 3));
    o[q].depth = __uint_as_float(e.x);
    o[q].bgr = e.y;
  }
  if (!tag_override && lin_tile == 0 && tid < CNT_SLOTS) k2_rearm_counters(st, tag, tid);
  if (depth) {
#pragma unroll
    for (int q = 0; q < K2_PPT; ++q)
      if (in_img[q]) depth[pix_i[q]] = o[q].depth;
  }
  if (bgr) {
    const bool full_rows = (tb.proj_w & 3) == 0 && (tile_x + 1) * K2_TW <= tb.proj_w;
    if (full_rows) {  // 3 * K2_TW contiguous bytes per tile row: assemble in LDS, store as dwords
#pragma unroll
      for (int q = 0; q < K2_PPT; ++q) {
        s_bgr[ty][(tx + q * K2_TX) * 3 + 0] = (uint8_t)(o[q].bgr & 0xff);
        s_bgr[ty][(tx + q * K2_TX) * 3 + 1] = (uint8_t)((o[q].bgr >> 8) & 0xff);
        s_bgr[ty][(tx + q * K2_TX) * 3 + 2] = (uint8_t)((o[q].bgr >> 16) & 0xff);
      }
      __syncthreads();
      constexpr int DW = K2_TW * 3 / 4;  // dwords per row
#pragma unroll
      for (int i0 = 0; i0 < K2_TY * DW; i0 += NT) {
        const int i = i0 + tid;
        if (i < K2_TY * DW) {
          const int r = i / DW, q = i - r * DW, vv = tile_y * K2_TY + r;
          if (vv < tb.proj_h)
            reinterpret_cast<u32*>(bgr + (size_t)((__umul24((u32)vv, (u32)tb.proj_w) + tile_x * K2_TW) * 3u))[q] =
                reinterpret_cast<const u32*>(&s_bgr[r][0])[q];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < K2_PPT; ++q)
        if (in_img[q]) {
          uint8_t* b = bgr + (u64)pix_i[q] * 3;
          b[0] = (uint8_t)(o[q].bgr & 0xff);
          b[1] = (uint8_t)((o[q].bgr >> 8) & 0xff);
          b[2] = (uint8_t)((o[q].bgr >> 16) & 0xff);
        }
    }
  }
  XM_K2STAMP(6);
}

template <int FMT = 0, int PPT = 2>
__global__ __launch_bounds__(K2_TX* K2_TY) void k_frame_proj_tiled(const u64* __restrict__ keys, DevTables tb,
                                                                  SlotState* st, u32 tag_override,
                                                                  const unsigned char* __restrict__ dirty,
                                                                  const ulonglong2* __restrict__ zero16,
                                                                  float* __restrict__ depth, uint8_t* __restrict__ bgr,
                                                                  int tile_cap, int col_lo = 0, int col_hi = 0) {
  // every kernel argument in one scalar round trip (see k_scatter_tiled); never true
  if ((long long)((u64)keys | (u64)tb.k2_tiles | (u64)tb.k2_pix | (u64)tb.k2_tiles1 | (u64)tb.k2_pix1 | (u64)tb.dlut | (u64)tb.pmap | (u64)st | (u64)dirty |
                  (u64)zero16 | (u64)depth | (u64)bgr |
                  (u64)(long long)(tb.proj_w | tb.proj_h | tb.rect_w | tb.rect_h | (int)tag_override)) < 0)
    return;
  if (col_hi > col_lo) {  // band-sharded finish (xm_shard_finish_u16_band): only the tiles whose patch is centred on a frame column
                          // of [col_lo, col_hi) -- the rank's band of the merged frame; tiles without a patch go with column 0
    const int4 rec = (PPT == 1 ? tb.k2_tiles1 : tb.k2_tiles)[xcd_contiguous(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y)];
    const int c = rec.z > 0 ? rec.x + (rec.z >> 1) : 0;
    if (c < col_lo || c >= col_hi) return;
  }
  frame_proj_tiled_body<FMT, PPT>(keys, tb, st, tag_override, dirty, zero16, depth, bgr, tile_cap,
                                  blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y);
}

// multi-frame launch: grid = (tiles_x, tiles_y, frames)
template <int FMT = 0, int COND = 0, int PPT = 2>
__global__ __launch_bounds__(K2_TX* K2_TY) void k_frame_proj_tiled_batch(const FrameDesc* __restrict__ descs, DevTables tb,
                                                                        const ulonglong2* __restrict__ zero16,
                                                                        int tile_cap) {
  // The tile's patch record does not depend on the frame: its load goes out together with the frame descriptor's (a block of
  // K2 is a chain of dependent round trips -- descriptor, record, patch -- and 55 % of its lifetime at full occupancy is spent
  // before the patch has arrived: tools/k2_timeline.py).  The never-true test keeps the compiler from sinking the load
  // behind the branch.
  if constexpr (COND == 1) {  // redo node of a captured batch: a few blocks per frame walk the frame's tiles (see k_scatter_tiled_batch)
    const FrameDesc d = descs[blockIdx.z];
    if (!d.valid || frame_skipped<COND>(d.st)) return;
    const u32 gx = ((u32)tb.proj_w + K2_TX * PPT - 1) / (K2_TX * PPT), gy = ((u32)tb.proj_h + K2_TY - 1) / K2_TY;
    for (u32 b = blockIdx.y * gridDim.x + blockIdx.x; b < gx * gy; b += gridDim.x * gridDim.y) {
      frame_proj_tiled_body<FMT, PPT>(d.key_frame, tb, d.st, 0u, nullptr, zero16, d.depth, d.bgr, tile_cap, b, gx, gy);
      __syncthreads();  // the next tile's patch overwrites the LDS this one's pixels have just read
    }
    return;
  }
  const u32 blk_lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int4 rec = (PPT == 1 ? tb.k2_tiles1 : tb.k2_tiles)[xcd_contiguous(blk_lin, gridDim.x * gridDim.y)];
  const FrameDesc d = descs[blockIdx.z];
  if (!d.valid || rec.w < 0) return;
  if (frame_skipped<COND>(d.st)) return;
  frame_proj_tiled_body<FMT, PPT>(d.key_frame, tb, d.st, 0u, nullptr, zero16, d.depth, d.bgr, tile_cap, blk_lin, gridDim.x,
                                  gridDim.y, &rec);
}

// camera view / plain per-pixel conversion of a frame of n_pixels cells -> depth + BGR
template <typename Cells>
__global__ __launch_bounds__(BLOCK) void k_frame_direct(Cells cells, u64 n_pixels, double p03, float z_near,
                                                        float z_far, SlotState* st, u32 tag_override, int use_tag,
                                                        const uint2* __restrict__ dlut, float* __restrict__ depth,
                                                        uint8_t* __restrict__ bgr) {
  const u64 pixel = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if constexpr (Cells::keyed) {
    if (use_tag) {
      const u32 tag = tag_override ? tag_override : st->tag_a;
      cells.tag = tag;
      if (!tag_override && blockIdx.x == 0 && threadIdx.x < CNT_SLOTS) {
        u32* c = st->cnt[(tag & 1) ^ 1][threadIdx.x];
        c[0] = c[1] = c[2] = c[3] = 0;
        if (threadIdx.x == 0) {
          st->tag_b = tag;
          if (u32* hf = st->host_flags) host_flag_store(hf + 1, tag);
        }
      }
    }
  }
  float d = 0.0f;
  if (pixel < n_pixels) d = cells.get((u32)pixel);
  PixelOut o;
  if (Cells::keyed && dlut) {  // fused path: integer disparity -> tabulated A5-A7 (see k_build_dlut)
    const uint2 e = dlut[(u32)d & 0xffffu];
    o.depth = __uint_as_float(e.x);
    o.bgr = e.y;
  } else {
    o = disparity_pixel(d, p03, z_near, z_far);
  }
  if (depth && pixel < n_pixels) depth[pixel] = o.depth;
  if (bgr) store_bgr_block(bgr, (u64)blockIdx.x * BLOCK, n_pixels, o.bgr);
}

// multi-frame launch of the camera-view frame kernel: grid = (blocks per frame, frames)
__global__ __launch_bounds__(BLOCK) void k_frame_direct_batch(const FrameDesc* __restrict__ descs, u64 n_pixels,
                                                              const uint2* __restrict__ dlut) {
  const FrameDesc d = descs[blockIdx.y];
  if (!d.valid) return;
  SlotState* st = d.st;
  const u32 tag = st->tag_a;
  if (blockIdx.x == 0 && threadIdx.x < CNT_SLOTS) {
    u32* c = st->cnt[(tag & 1) ^ 1][threadIdx.x];
    c[0] = c[1] = c[2] = c[3] = 0;
    if (threadIdx.x == 0) {
      st->tag_b = tag;
      if (u32* hf = st->host_flags) host_flag_store(hf + 1, tag);
    }
  }
  const u64 pixel = (u64)blockIdx.x * BLOCK + threadIdx.x;
  u32 dsp = 0;
  if (pixel < n_pixels) dsp = key_disp(d.key_frame[pixel], tag);
  const uint2 e = dlut[dsp];
  if (d.depth && pixel < n_pixels) d.depth[pixel] = __uint_as_float(e.x);
  if (d.bgr) store_bgr_block(d.bgr, (u64)blockIdx.x * BLOCK, n_pixels, e.y);
}

// camera view on the compact key frame ((event index + 1) << 12 | disparity, 0 = no event): the pixel is zeroed once read, so
// the next frame of the slot starts from an empty frame without a clear of its own.  The frame is COLUMN-major
// (u32[cam_w][cam_h]: K1's flush walks consecutive rows of one window column -- 64 lanes = 256 contiguous bytes per atomic
// instruction instead of four 64-byte row pieces), the outputs are row-major: a block takes a 32 x 32-pixel tile, reads it
// along the columns, hands the 12-bit disparities over through LDS and writes rows (128 bytes of depth, 96 of BGR per row).
// (CAM32_T: xmaps_geometry.hpp)
__device__ __forceinline__ void frame_cam32_body(u32* __restrict__ frame32, const int cam_w, const int cam_h, SlotState* st,
                                                 const uint2* __restrict__ dlut, float* __restrict__ depth, uint8_t* __restrict__ bgr,
                                                 const u32 tile_x, const u32 tile_y) {
  __shared__ uint16_t s_d[CAM32_T][CAM32_T + 2];
  __shared__ __attribute__((aligned(16))) uint8_t s_b[CAM32_T][CAM32_T * 3];
  const int tid = threadIdx.x, lo = tid & (CAM32_T - 1), hi = tid / CAM32_T;  // BLOCK / 32 = 8 columns (rows) per pass
  if (tile_x == 0 && tile_y == 0 && tid < CNT_SLOTS) {
    const u32 tag = st->tag_a;
    u32* c = st->cnt[(tag & 1) ^ 1][tid];
    c[0] = c[1] = c[2] = c[3] = 0;
    if (tid == 0) {
      st->tag_b = tag;
      if (u32* hf = st->host_flags) host_flag_store(hf + 1, tag);
    }
  }
  const int x0 = (int)tile_x * CAM32_T, y0 = (int)tile_y * CAM32_T;
#pragma unroll
  for (int i = 0; i < CAM32_T * CAM32_T / BLOCK; ++i) {  // lanes = consecutive rows of one frame column
    const int c = hi + i * (BLOCK / CAM32_T), x = x0 + c, y = y0 + lo;
    u32 k = 0;
    if (x < cam_w && y < cam_h) {
      u32* p = frame32 + (u32)x * (u32)cam_h + (u32)y;
      k = *p;
      if (k) *p = 0u;
    }
    s_d[c][lo] = (uint16_t)(k & 0xfffu);
  }
  __syncthreads();
  const bool dw_rows = bgr && (cam_w & 3) == 0 && x0 + CAM32_T <= cam_w && ((size_t)bgr & 3) == 0;  // whole 96-byte rows, dword aligned
#pragma unroll
  for (int i = 0; i < CAM32_T * CAM32_T / BLOCK; ++i) {  // lanes = consecutive pixels of one output row
    const int r = hi + i * (BLOCK / CAM32_T), x = x0 + lo, y = y0 + r;
    const uint2 e = dlut[s_d[lo][r]];
    if (x < cam_w && y < cam_h) {
      const u32 pixel = (u32)y * (u32)cam_w + (u32)x;
      if (depth) depth[pixel] = __uint_as_float(e.x);
      if (bgr && !dw_rows) {
        bgr[(size_t)pixel * 3 + 0] = (uint8_t)(e.y & 0xff);
        bgr[(size_t)pixel * 3 + 1] = (uint8_t)((e.y >> 8) & 0xff);
        bgr[(size_t)pixel * 3 + 2] = (uint8_t)((e.y >> 16) & 0xff);
      }
    }
    if (dw_rows) {
      s_b[r][lo * 3 + 0] = (uint8_t)(e.y & 0xff);
      s_b[r][lo * 3 + 1] = (uint8_t)((e.y >> 8) & 0xff);
      s_b[r][lo * 3 + 2] = (uint8_t)((e.y >> 16) & 0xff);
    }
  }
  if (dw_rows) {
    __syncthreads();
    constexpr int DW = CAM32_T * 3 / 4;  // dwords per staged row
    for (int i = tid; i < CAM32_T * DW; i += BLOCK) {
      const int r = i / DW, q = i - r * DW, y = y0 + r;
      if (y < cam_h) reinterpret_cast<u32*>(bgr + ((size_t)y * (size_t)cam_w + (size_t)x0) * 3)[q] = reinterpret_cast<const u32*>(&s_b[r][0])[q];
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_frame_cam32(u32* __restrict__ frame32, int cam_w, int cam_h, SlotState* st,
                                                       const uint2* __restrict__ dlut, float* __restrict__ depth,
                                                       uint8_t* __restrict__ bgr) {
  frame_cam32_body(frame32, cam_w, cam_h, st, dlut, depth, bgr, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(BLOCK) void k_frame_cam32_batch(const FrameDesc* __restrict__ descs, int cam_w, int cam_h,
                                                             const uint2* __restrict__ dlut) {
  const FrameDesc d = descs[blockIdx.z];
  if (!d.valid) return;
  frame_cam32_body(reinterpret_cast<u32*>(d.key_frame), cam_w, cam_h, d.st, dlut, d.depth, d.bgr, blockIdx.x, blockIdx.y);
}

// Sharded frames: a chunk of the (reduced) packed-key frame -> u16 disparities (0 where the tag differs): 2 instead of 8
// bytes per cell for the all-gather that follows the reduce-scatter
__global__ __launch_bounds__(BLOCK) void k_decode_keys_u16(const u64* __restrict__ f, u64 n_cells, u32 tag, uint16_t* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n_cells) out[i] = key_disp(f[i], tag);
}

// camera view on a plain u16 disparity frame
__global__ __launch_bounds__(BLOCK) void k_frame_direct_u16(const uint16_t* __restrict__ disp, u64 n_pixels,
                                                            const uint2* __restrict__ dlut, float* __restrict__ depth,
                                                            uint8_t* __restrict__ bgr) {
  const u64 pixel = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const uint2 e = dlut[pixel < n_pixels ? (u32)disp[pixel] : 0u];
  if (depth && pixel < n_pixels) depth[pixel] = __uint_as_float(e.x);
  if (bgr) store_bgr_block(bgr, (u64)blockIdx.x * BLOCK, n_pixels, e.y);
}

}  // namespace xm
