// The fp16 MFMA tile-sweep core shared by the certified E-step filter
// (estep_x64_kernel, estep_f32.hip) and the IPE screens (ipe16_sweep_kernel /
// ipe16_values_kernel, ipe16.hip): the fp16 hi/lo centroid operand's byte
// layout, the 3-slot LDS ring it is staged through, the wave's resident
// row-set A fragments and the half-tile MFMA pass.  Everything is
// force-inlined and takes the per-lane register arrays by reference, indexed
// by compile-time constants only: the kernels on top sit at the register
// limit, and the ring's counted vmcnt assumes no scratch traffic between a
// DMA and its wait.
#pragma once
#include "common.h"
#include <utility>

namespace sq {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileN = 64;          // centroids per LDS tile

SQ_DEV float vmin(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// (bits(a) & m) | q in ONE VALU op (v_and_or_b32; the compiler emits an and
// plus an or3 that it pairs across values)
SQ_DEV float and_or(float a, uint32_t m, uint32_t q) {
  float r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(m), "v"(q));   // one SGPR per VOP3 on gfx9
  return r;
}
SQ_DEV float vmed3(float a, float b, float c) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

template <typename F, int... I>
SQ_DEV void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
SQ_DEV void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// C/D layout of v_mfma_f32_32x32x16: accumulator register i of lane
// (half, r32) holds this row of the wave's 32 (column r32 of the 32)
__host__ __device__ constexpr int acc_row(int i, int half) {
  return (i & 3) + 8 * (i >> 2) + 4 * half;
}

// ---------------------------------------------------------------------------
// The operand.  Per 64-centroid tile: [hi chunks: d_pad / 8 + 2, the last two
// the norm step][lo chunks: d_pad / 8], a chunk = [64 centroids][8 fp16]
// (1 KiB, one LDS-DMA piece).  A k-step (16 features) is a chunk pair: lane
// half 0 reads features 0-7, half 1 features 8-15, of centroid r32 (column
// half 0) or 32 + r32 (column half 1), so every B-fragment read is lane base
// + immediate.  The norm step holds the 3-way fp16 split of alpha^2 |c|^2 at
// features d_pad .. d_pad + 2 (against the A fragment [1, 1, 1, 0 ...]),
// zeros after.
namespace f16op {
constexpr int kChunkElems = kTileN * 8;            // fp16 elements per chunk
constexpr int kChunkBytes = kChunkElems * 2;       // = one LDS-DMA piece (64 lanes x 16 B)
constexpr int kStepBytes = 2 * kChunkBytes;        // one k-step of a tile
constexpr int kColHalfBytes = 32 * 16;             // centroid 32 + r32 from centroid r32
constexpr int kNormElems = 3;                      // features d_pad .. d_pad + 2

// bytes of a tile's hi region (data + norm k-steps) / of a whole tile
__host__ __device__ constexpr int hi_bytes(int ksd) { return (ksd + 1) * kStepBytes; }
__host__ __device__ constexpr int tile_bytes(int ksd) { return (2 * ksd + 1) * kStepBytes; }

// writers: element of (centroid j, feature f) = row_base(d_pad, j) + hi_off(f)
// (f < d_pad + 16: the norm step included) or + lo_off(d_pad, f) (f < d_pad)
__host__ __device__ constexpr size_t row_base(int d_pad, int j) {
  return (size_t)(j >> 6) * (2 * (d_pad / 8) + 2) * kChunkElems + (size_t)(j & 63) * 8;
}
__host__ __device__ constexpr size_t hi_off(int f) { return (size_t)(f >> 3) * kChunkElems + (f & 7); }
__host__ __device__ constexpr size_t lo_off(int d_pad, int f) {
  return (size_t)(d_pad / 8 + 2 + (f >> 3)) * kChunkElems + (f & 7);
}

// readers: the lane's byte offset in a tile, and from there its B fragment of
// (column half h, k-step ks) of the hi region
__host__ __device__ constexpr int lane_off(int half, int r32) { return (half * 64 + r32) * 16; }
__host__ __device__ constexpr int frag_off(int h, int ks) { return h * kColHalfBytes + ks * kStepBytes; }
}  // namespace f16op

SQ_DEV f16x8 ldb(const unsigned char* p) { return *reinterpret_cast<const f16x8*>(p); }

// ---------------------------------------------------------------------------
// The ring.  A tile's hi region is KT = KSD + 1 k-steps.  Up to d_pad = 256 a
// whole tile is one LDS slot; above, the tile is staged in NS sub-tiles of at
// most 24 k-steps (48 KiB) so the 3 slots stay within the 160 KiB LDS at
// every d_pad <= 1024.  Staging runs two units ahead: sync() retires the unit
// staged one step earlier and leaves the last stage()'s PPW loads per wave in
// flight across the raw s_barrier (no __syncthreads: its fence would drain
// them).
template <int KSD, int NW>
struct TileRing {
  static constexpr int RING = 3;                        // LDS slots (2 units in flight)
  static constexpr int KT = KSD + 1;
  static constexpr int NS = (KT + 23) / 24;
  static constexpr int SK = (KT + NS - 1) / NS;         // k-steps per slot
  static constexpr int SLOT = SK * f16op::kStepBytes;   // bytes per LDS slot
  static constexpr int PIECES = SLOT / f16op::kChunkBytes;   // LDS-DMA pieces per slot
  static constexpr int PPW = (PIECES + NW - 1) / NW;    // loads per wave per stage (uniform: counted vmcnt)
  static constexpr int BYTES = RING * SLOT;

  static SQ_DEV unsigned char* buf(unsigned char* smem, int g) { return smem + (g % RING) * SLOT; }

  // unit U = sub-tile U % NS of tile (U / NS) % n_tiles (the sequence runs on
  // across row blocks); for workgroups of NW waves in x
  static SQ_DEV void stage(const _Float16* C, unsigned char* smem, int U, int n_tiles) {
    const int t = (NS == 1 ? U : U / NS) % n_tiles;
    const int sub = NS == 1 ? 0 : U % NS;
    const int npc = 2 * min(SK, KT - sub * SK);   // valid pieces of this sub-tile
    const unsigned char* tile = reinterpret_cast<const unsigned char*>(C) +
                                (size_t)t * f16op::tile_bytes(KSD) + (size_t)sub * SLOT;
    unsigned char* dst = buf(smem, U);
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      // every wave issues PPW loads (the surplus repeat the last piece: same
      // bytes to the same LDS slot) so one counted vmcnt fits all waves.
      // (wave and lane derived here, at their use: passed in as arguments
      // the compiler folds the address in another order and the kernels on
      // top gain SGPR spills - estep_x64 <16, 2>: 27 against 1 this way)
      const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
      const int p = wave + NW * i < npc ? wave + NW * i : npc - 1;
      const int lane = threadIdx.x & 63;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(tile + p * f16op::kChunkBytes + lane * 16),
          (__attribute__((address_space(3))) void*)(dst + p * f16op::kChunkBytes), 16, 0, 0);
    }
  }
  static SQ_DEV void sync() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
    __builtin_amdgcn_s_barrier();
  }
};

// resident workgroups of a persistent kernel: CUs x blocks per CU
static inline int resident_blocks(const void* kern, int threads, size_t lds) {
  int dev = 0, cus = 0, per_cu = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds);
  return (cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
}

// ---------------------------------------------------------------------------
// The row-set operand: RS sets of 32 rows per wave, lane (half, r32) holding
// features 8 half .. 8 half + 7 of every k-step of row r32 of each set.
// row(st): pointer to the fp16 row that the lane holds of set st (the row at
// position (wave RS + st) 32 + r32 of the block).
SQ_DEV f16x8 a_frag(const _Float16* row, int half, int ks) {
  return *reinterpret_cast<const f16x8*>(row + half * 8 + ks * 16);
}
template <int RS, int KSD, typename Row>
SQ_DEV void load_a(f16x8 (&ah)[RS][KSD], int half, Row&& row) {
#pragma unroll
  for (int st = 0; st < RS; ++st) {
    const _Float16* xr = row(st);
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) ah[st][ks] = a_frag(xr, half, ks);
  }
}
// the A fragment of the norm step
SQ_DEV f16x8 aug_frag(int half) {
  f16x8 aug = (f16x8)0;
  if (half == 0) { aug[0] = aug[1] = aug[2] = (_Float16)1.0f; }
  return aug;
}

// ---------------------------------------------------------------------------
// The half-tile pass.  The two column halves of a tile (cur: its LDS slot) are
// one stream of 2 KT B fragments through a ring of PFD + 1 registers, read
// PFD k-steps ahead of their MFMAs, so the second half's first reads are in
// flight during the first half's last MFMAs; tile_prime() issues the first
// PFD reads of a tile.  Pass H accumulates column half H of all RS row sets
// from zero while epi(st, i, o[st][i], qo) of the previous half-tile (o) is
// spread evenly over the KT k-steps.
template <int KT, int NB>
SQ_DEV void tile_prime(const unsigned char* cur, int lane_off, f16x8 (&bq)[NB]) {
#pragma unroll
  for (int j = 0; j < NB - 1; ++j) bq[j] = ldb(cur + lane_off + f16op::frag_off(j / KT, j % KT));
}
template <int H, int KSD, int RS, int NB, typename Epi>
SQ_DEV void half_pass(const unsigned char* cur, int lane_off, const f16x8 (&ah)[RS][KSD],
                      const f16x8& aug, f16x8 (&bq)[NB], f32x16 (&acc)[RS],
                      const f32x16 (&o)[RS], uint32_t qo, bool do_epi, Epi&& epi) {
  constexpr int KT = KSD + 1, PFD = NB - 1;
#pragma unroll
  for (int st = 0; st < RS; ++st) acc[st] = (f32x16){0};
#pragma unroll
  for (int ks = 0; ks < KT; ++ks) {
    const int g = H * KT + ks;
    if (g + PFD < 2 * KT)
      bq[(g + PFD) % NB] = ldb(cur + lane_off + f16op::frag_off((g + PFD) / KT, (g + PFD) % KT));
#pragma unroll
    for (int st = 0; st < RS; ++st)
      acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks < KSD ? ah[st][ks] : aug, bq[g % NB],
                                                       acc[st], 0, 0, 0);
    if (do_epi) {
#pragma unroll
      for (int e = (ks * 16 * RS) / KT; e < ((ks + 1) * 16 * RS) / KT; ++e)
        epi(e / 16, e % 16, o[e / 16][e % 16], qo);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
// every value of a half-tile through epi (the last half-tile of a sweep)
template <int RS, typename Epi>
SQ_DEV void half_drain(const f32x16 (&o)[RS], uint32_t qo, Epi&& epi) {
#pragma unroll
  for (int st = 0; st < RS; ++st)
#pragma unroll
    for (int i = 0; i < 16; ++i) epi(st, i, o[st][i], qo);
}

// Both column halves of one tile (tile: its first byte, LDS or global) for
// one row set from zero: the pass's operands (a_frag / aug_frag against
// frag_off) in the pass's k-step order through the same MFMA, so c0 / c1
// equal the pass's accumulators bit for bit.  ksd may be a runtime value.
SQ_DEV void tile_from_zero(const unsigned char* tile, int lane_off, const _Float16* row, int half,
                           int ksd, f32x16& c0, f32x16& c1) {
  const f16x8 aug = aug_frag(half);
  c0 = (f32x16){0};
  c1 = (f32x16){0};
  for (int ks = 0; ks < ksd + 1; ++ks) {
    const f16x8 av = ks < ksd ? a_frag(row, half, ks) : aug;
    const f16x8 b0 = ldb(tile + lane_off + f16op::frag_off(0, ks));
    const f16x8 b1 = ldb(tile + lane_off + f16op::frag_off(1, ks));
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b0, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b1, c1, 0, 0, 0);
  }
}

}  // namespace sq
