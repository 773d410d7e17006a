// Weight-gradient GEMM for the fused MLPs: dW[o][i] (+)= sum over points p of A[o,p] * B[i,p], with A and B
// stored as wave-tile activation blocks (svs_mlp.hip: 256 feature rows x 32 points per block, float4 index
// (i/4)*64+lane).  This is the "K = number of points" contraction of the training backward
// (d loss / d W_l = a_bar_l h_l^T + g_hat_l u_l^T).
//
// One workgroup (4 waves, one per SIMD) owns a full 256 x (32*NTB) accumulator (wave w: output tiles 2w, 2w+1 x
// all input tiles) and walks over its share of the (point tile, operand pair) items -- split-K over workgroups.
// An item's A and B blocks are staged global -> registers -> LDS as [point][feature] rows of pitch 260/292 floats:
// a lane's float4 (4 consecutive features of one point) is ONE conflict-free ds_write_b128, and the MFMA operand
// reads (32 consecutive features of one point per half-wave) are conflict-free ds_read_b32.  The loads of item i+1
// are in flight while item i's MFMAs run (two LDS buffers, one barrier per item).  Partial sums are flushed with
// float atomics, two 128-byte row segments per wave-instruction (the full-rate shape, MI355X_MICROARCH.md
// "Global float atomics").
#include "svs_common.h"
#include "svs_mlp_layout.h"
#include "svs_ticket.h"
#include "svs_wgrad_maps.h"
#include <cstdlib>
#include <type_traits>

namespace svs {
namespace wgrad {

struct Pair {
  const float* a;        // blocks [n_tiles][stride_a]: A rows (gradients w.r.t. layer outputs)
  const float* b;        // blocks: B rows (layer inputs)
  size_t stride_a, stride_b;   // floats between consecutive point tiles
};

struct Args {
  Pair p[2];
  int n_pairs;
  int n_tiles;           // point tiles (32 points each)
  int n_valid_points;    // points beyond this index contribute nothing (ragged last tile)
  const float* b_extra;  // optional 9th B tile: [n_tiles][stride_extra], 16 registers x 64 lanes (pair 0 only)
  size_t stride_extra;
  float* dW;             // [256][ldw] accumulated with atomics (caller zeroes)
  int ldw;
  float* db;             // [256] row sums of A of pair 0 (bias gradient) or nullptr
  det::Ticket ticket;    // deterministic mode: the workgroups flush in block order (svs_ticket.h)
};

struct Staging {
  f32x4 a[8], b[8], x;
};

template <int NTB>
__global__ __launch_bounds__(256, 1) void wgrad_kernel(Args a) {
  constexpr int PA = 260, PB = NTB == 9 ? 292 : 260;       // row pitches (floats), both = 4 mod 32
  constexpr int BUF = 32 * (PA + PB);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, col = lane & 31;
  f32x16 acc[2][NTB];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < NTB; ++i) acc[o][i] = (f32x16)(0.0f);
  float bias_acc = 0.0f;

  const int my_tiles = a.n_tiles > (int)blockIdx.x ? (a.n_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  const int n_items = my_tiles * a.n_pairs;
  Staging st;
  int st_live = 32;

  auto issue = [&](int item) {
    const int t = blockIdx.x + (item / a.n_pairs) * gridDim.x, pi = item % a.n_pairs;
    const Pair& p = a.p[pi];
    const f32x4* ga = reinterpret_cast<const f32x4*>(p.a + (size_t)t * p.stride_a);
    const f32x4* gb = reinterpret_cast<const f32x4*>(p.b + (size_t)t * p.stride_b);
#pragma unroll
    for (int k = 0; k < 8; ++k) { st.a[k] = ga[k * 256 + tid]; st.b[k] = gb[k * 256 + tid]; }
    if (NTB == 9) {
      st.x = (a.b_extra && pi == 0) ? reinterpret_cast<const f32x4*>(a.b_extra + (size_t)t * a.stride_extra)[tid]
                                    : (f32x4)(0.0f);
    }
    st_live = a.n_valid_points - t * 32;
  };
  auto commit = [&](int buf) {
    float* la = smem + buf * BUF;
    float* lb = la + 32 * PA;
    if (st_live < 32) {
      // ragged last tile: points beyond the batch contribute nothing
#pragma unroll
      for (int k = 0; k < 8; ++k) if ((tid & 31) >= st_live) st.a[k] = (f32x4)(0.0f);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int q = k * 256 + tid, i4 = q >> 6, ln = q & 63;
      const int feat = 32 * (i4 >> 2) + 8 * (i4 & 3) + 4 * (ln >> 5), pt = ln & 31;
      *reinterpret_cast<f32x4*>(la + pt * PA + feat) = st.a[k];
      *reinterpret_cast<f32x4*>(lb + pt * PB + feat) = st.b[k];
    }
    if (NTB == 9) {
      const int i4 = tid >> 6, ln = tid & 63;
      *reinterpret_cast<f32x4*>(lb + (ln & 31) * PB + 256 + 8 * i4 + 4 * (ln >> 5)) = st.x;
    }
  };

  if (n_items > 0) { issue(0); commit(0); }
  __syncthreads();
  for (int item = 0; item < n_items; ++item) {
    const int buf = item & 1;
    const bool more = item + 1 < n_items;
    if (more) issue(item + 1);
    const float* la = smem + buf * BUF;
    const float* lb = la + 32 * PA;
    if (a.db && (item % a.n_pairs) == 0) {
      float s = 0.0f;
#pragma unroll 8
      for (int q = 0; q < 32; ++q) s += la[q * PA + tid];
      bias_acc += s;
    }
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const int pt = 2 * s + half;
      const float a0 = la[pt * PA + 32 * (2 * wave) + col];
      const float a1 = la[pt * PA + 32 * (2 * wave + 1) + col];
#pragma unroll
      for (int i = 0; i < NTB; ++i) {
        const float b = lb[pt * PB + 32 * i + col];
        acc[0][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][i], 0, 0, 0);
        acc[1][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][i], 0, 0, 0);
      }
    }
    if (more) commit(buf ^ 1);
    __syncthreads();
  }
  // flush: C[row = rho(r) + 4*half][col]; two 128-byte row segments per wave-instruction
  det::wait_turn(a.ticket, blockIdx.x);
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < NTB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * (2 * wave + o) + rho(r) + 4 * half;
        const int c = 32 * i + col;
        if (c < a.ldw) atomicAdd(&a.dW[(size_t)row * a.ldw + c], acc[o][i][r]);
      }
  if (a.db) atomicAdd(&a.db[tid], bias_acc);
  det::pass_turn(a.ticket, blockIdx.x);
}


// --------------------------------------------------------------------------------------------------------------
// fp16x2 variant: the same contraction on v_mfma_f32_16x16x32_f16, reading the operand blocks in the forms the sweeps
// store them in (svs_blocks_h2.h): no conversion, no split, no staging registers.
//   pair 0:  A = abar_l / zbar_l / fbar  scaled block, per-point scale
//            B = h_l / r_l / feature     pair block
//   pair 1:  A = ghat_l                  stored unscaled
//            B = u_l                     scaled block, per-point scale
//   narrow:  B = the 16 / 32 extra input rows of a radiance network's first layer, ONE float32 tile (split here)
// GP = true (precision SVS_MMA_F16X2): every operand with both fp16 pieces, three MFMAs per 16 x 16 output tile and item (hi
// mid + mid hi + hi hi: the float32 accuracy class), 64 KiB per item, a ring of 2 item slots.
// GP = false (SVS_MMA_F16X2_HALF): hi planes only (the scaled blocks hold nothing else), one MFMA, 32 KiB per item, a ring
// of 4 slots with 3 items in flight.
//
// The contraction index is the POINT, which lives on the lanes of the fragments.  A 16-KiB plane is copied into LDS as it
// stands by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction) into a ring of four item slots (A plane, B
// plane), three items ahead of the one being multiplied.  One MFMA contracts a whole 32-point tile: a wave's 32 rows x 256
// columns are 2 row tiles x 16 column tiles of 16 x 16 (32 accumulators of 4 registers), 2 x 16 x 3 MFMAs per item, every B
// fragment feeding both row tiles.  The MFMA fragments (one feature, 8 points per lane; lane group g = lane >> 4 selects WHICH
// 8 points) are read TRANSPOSED out of the plane with ds_read_b64_tr_b16 (16 lanes: 16 features x 4 points), two reads per
// fragment.  The order of the points inside the contraction is free as long as A, B and the factor table agree, and is chosen
// for the banks: with the slot permutation of the planes (piece_slot(), svs_blocks_h2.h)
//     byte = 1024 s + 256 (a >> 1) + 128 ((a & 1) ^ (s & 1)) + 64 (p & 1) + 16 q + 8 (p >> 1)
// (s = feature / 16 = the tile, shared by all four lane groups; a = point / 4, q = point % 4, p = the lane's column quad) lane
// groups 0, 1, 2, 3 take the point quads {0, 2}, {1, 3}, {4, 6}, {5, 7}: the two groups of a 32-lane half differ in the parity
// of a and hit 32 distinct 8-byte slots of one 256-byte line.  The maps are the constexpr functions of svs_wgrad_maps.h, where
// this is proved for every read of the loop by static_assert.  (Why this shape and not 32x32x16, on which the kernel was bound
// by its multiply phase at the clock the chip holds under that load; the flush measured; 64 x 128 wave tiles built and
// dropped: DESIGN.md section 4, profiles/wgrad_shape.txt.)
//
// Scaled operands carry value * s_p with one power of two s_p per point (the point's largest element at ~2^4); a
// contraction over points needs ONE scale, so every A fragment is multiplied by the factors s / s_p of its 8 points (a table
// in the fragments' point order, maps::factor_pos) in fp16 (exact: powers of two) -- for pair 1 the factors of B's points
// are applied to A, which is the same product -- with
// s chosen from the published maximum of the scaled operand (absmax) so that the largest element of the launch is
// ~2^10; the accumulators are multiplied by 1 / s before the flush.  Factors are clamped to 2^15; points beyond the
// batch get factor 0.
// --------------------------------------------------------------------------------------------------------------
namespace h2 {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
#define SVS_LDS(T, ptr) ((__attribute__((address_space(3))) T*)(ptr))

constexpr int kPlane = 16384;          // bytes of one fp16 plane of a block (svs_blocks_h2.h)
constexpr int kExtraPiece = 32 * 64;   // narrow B tile: [2 column tiles][32 points][16 features] fp16, 32-byte rows (hi, then mid)
constexpr int kNarrowImg = 8192;       // a narrow job has no B plane: its float32 B tile lands (LDS-DMA) at the B plane's
                                       // place, its fp16 image (hi, mid) kNarrowImg bytes further
constexpr int kRecBytes = 8 * 256;     // per ring slot: every wave's copy of the scaled operand's record (64 floats)
constexpr int kFactorBytes = 8 * 64;   // per ring slot: 8 waves x 32 fp16 factors
template <bool GP>
struct Ring {
  static constexpr int kPlanes = GP ? 2 : 1;            // planes per operand
  static constexpr int kSlot = 2 * kPlanes * kPlane;    // ring slot: A plane(s), B plane(s)
  static constexpr int kB = kPlanes * kPlane;           // offset of the B planes inside a slot
  static constexpr int kRing = GP ? 2 : 4;
  static constexpr int kAhead = kRing - 1;              // items in flight beyond the one being multiplied
  static constexpr int kSlotAll = kSlot + kRecBytes + kFactorBytes;
  static constexpr int kLdsBytes = kRing * kSlotAll;
};

// LDS reads of the main loop go through inline asm: hipcc's waitcnt pass makes every LDS access it can see wait for ALL
// LDS-DMA in flight (vmcnt(0): it cannot tell the ring slots apart), which would un-pipeline the ring.  The reads are
// ordered against the copies by the counted vmcnt waits + barriers of the loop; lds_wait() is the lgkmcnt side.
// A fragment is two transposed reads 256 bytes apart (the lane group's two point quads, svs_wgrad_maps.h); everything that is
// the same for all lanes goes into the instruction's offset field, so an item's reads share a handful of base registers.
struct Frag { s16x4 lo, hi; };
template <int OFF>
__device__ __forceinline__ void tr_issue(Frag& v, unsigned base) {
  static_assert(OFF >= 0 && OFF + 256 < 65536, "ds offset field");
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v.lo) : "v"(base), "n"(OFF));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v.hi) : "v"(base), "n"(OFF + 256));
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): loops whose index ends up in an offset field
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}
__device__ __forceinline__ f16x8 frag_of(const Frag& v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ void lds_read128(f32x4& v, unsigned a) { asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a)); }
__device__ __forceinline__ void lds_read32(float& v, unsigned a) { asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(a)); }
__device__ __forceinline__ void lds_wait() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);      // hipcc hoists register-only MFMAs above an asm wait otherwise (rule 18)
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(unsigned long long)SVS_LDS(const void, p);
}

// power-of-two scale from the maximum magnitude: s * absmax in [2^14, 2^15) -- as high as fp16 allows (the re-scaled A
// fragments of points whose gradients are far below the launch's maximum go subnormal in fp16: every bit of range above
// them is a bit of precision for those points)
__device__ __forceinline__ void scale_from_absmax(const float* absmax, float& s, float& inv_s) {
  s = 1.0f; inv_s = 1.0f;
  if (!absmax) return;
  int e = (int)((__float_as_uint(*absmax) >> 23) & 0xff);
  e = e < 16 ? 16 : (e > 250 ? 250 : e);
  s = __uint_as_float((unsigned)(268 - e) << 23);
  inv_s = __uint_as_float((unsigned)(e - 14) << 23);
}

// One launch covers a list of jobs (the weight gradients of several layers): each job gets a contiguous range of
// workgroups, proportional to its work, which split its point tiles among themselves -- about one workgroup per CU
// in total, so the number of partial sums flushed with atomics per layer is ~256 / n_jobs instead of 256.
struct Job {
  Pair p[2];
  const float* rec[2];   // per pair: the records [tile][64] of its scaled operand (pair 0: A, pair 1: B), or nullptr
  int n_pairs;
  int n_tiles;           // point tiles (32 points each)
  int n_valid_points;    // points beyond this index contribute nothing (ragged last tile)
  int b_tiles;           // 8: B blocks are 256-row blocks; 1: B blocks are single 32-row float32 tiles (1024 floats)
  int col0;              // first dW column of B tile 0
  float* dW;             // [256][ldw] accumulated with atomics (caller zeroes)
  int ldw;
  float* db;             // [256] row sums of A of pair 0 (bias gradient) or nullptr
  const float* absmax;   // device float: max magnitude of the scaled operands, or nullptr (scales ignored)
  int wg_begin, wg_count;
  det::Ticket ticket;    // deterministic mode: the workgroups that add into this job's dW columns flush in turn (svs_ticket.h)
};
constexpr int kMaxJobs = 20;
struct MultiArgs { Job job[kMaxJobs]; int n_jobs; int touch; int reverse; };
static_assert(sizeof(MultiArgs) <= 4096, "kernel arguments");

// 8 waves: wave w owns output rows 32 w .. 32 w + 31 x all 256 columns, as kRT x kCT tiles of 16 x 16 -- 32 accumulators
// of 4 registers
constexpr int kThreadsW = 512;
constexpr int kRT = 2, kCT = 16;
// the bank-conflict proof of every transposed read of the loop (svs_wgrad_maps.h), with the regions the reads are offset by
static_assert(maps::plane_reads_ok(kPlane), "transposed reads of the operand planes: bank conflict");
static_assert(maps::narrow_reads_ok(kExtraPiece), "transposed reads of the narrow B image: bank conflict");
static_assert(kPlane % 256 == 0 && kNarrowImg % 256 == 0 && kExtraPiece % 256 == 0 && Ring<true>::kSlotAll % 256 == 0 &&
              Ring<false>::kSlotAll % 256 == 0, "every region the reads are offset by starts on a 256-byte bank row");

typedef const __attribute__((address_space(1))) void* gvoid;

template <bool GP>
__global__ __launch_bounds__(kThreadsW, 1) void wgrad_h2_multi_kernel(MultiArgs ma) {
  typedef Ring<GP> R;
  constexpr int kSlot = R::kSlot, kSlotAll = R::kSlotAll, kRing = R::kRing, kAhead = R::kAhead, kB = R::kB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_h2[];
  int jj = 0;
  for (int q = 1; q < ma.n_jobs; ++q) if ((int)blockIdx.x >= ma.job[q].wg_begin) jj = q;
  const Job& a = ma.job[jj];
  const int wg = (int)blockIdx.x - a.wg_begin, nwg = a.wg_count;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool narrow = a.b_tiles == 1;
  float s_grad, inv_s;
  scale_from_absmax(a.absmax, s_grad, inv_s);

  f32x4 acc[kRT][kCT];
#pragma unroll
  for (int o = 0; o < kRT; ++o)
#pragma unroll
    for (int i = 0; i < kCT; ++i) acc[o][i] = (f32x4)(0.0f);
  float bsum[kRT];       // bias gradient: this lane's row (lane & 15 of row tile o) over its lane group's 8 points
#pragma unroll
  for (int o = 0; o < kRT; ++o) bsum[o] = 0.0f;

  unsigned char* ring = smem_h2;

  // ---- transposed-read addresses (svs_wgrad_maps.h): the lane's part for even and for odd tiles of a plane and the wave's
  // first row tile of A; tile number, plane and the fragment's second read are offset fields
  const int rg = lane >> 4;
  const int rd_even = maps::plane_base(0, lane), rd_odd = maps::plane_base(1, lane);
  const int a_off = 1024 * kRT * wave;
  const int rx = maps::narrow_base(lane);
  // narrow B image writer (threads 0..255): float4 tid of the float32 tile = registers 4 (tid >> 6) .. +3 of lane tid & 63,
  // features 8 (tid >> 6) + 4 (lane >> 5) .. + 3 of point lane & 31
  const int wp = lane & 31, whf = lane >> 5;
  const int wxoff = maps::narrow_at(8 * (wave & 3) + 4 * whf, wp);
  // column tiles of the job: a narrow job's 32 columns are two
  const int n_ct = narrow ? 2 : kCT;

  const bool two_pairs = a.n_pairs == 2;               // (1 or 2)
  const int my_tiles = a.n_tiles > wg ? (a.n_tiles - 1 - wg) / nwg + 1 : 0;
  const int n_items = two_pairs ? 2 * my_tiles : my_tiles;
  const int n_valid = a.n_valid_points;
  const bool has_db = a.db != nullptr;
  // the point tile of an item.  ma.reverse (experiment, SVS_WGRAD_REVERSE=1): the tiles in DESCENDING order -- the sweep that ran
  // just before this launch wrote and read the highest tiles last, so the GEMM would start on what may still sit in the 256 MB
  // Infinity Cache
  const bool rev = ma.reverse != 0;
  // (the job's operand pointers and strides in registers: read through `a` -- kernel-argument memory -- inside issue() they were
  // scalar loads per item, each waited for with lgkmcnt(0), in front of the copies)
  const float* const pa0 = a.p[0].a; const float* const pb0 = a.p[0].b;
  const float* const pa1 = a.p[1].a; const float* const pb1 = a.p[1].b;
  const size_t sa0 = a.p[0].stride_a, sb0 = a.p[0].stride_b, sa1 = a.p[1].stride_a, sb1 = a.p[1].stride_b;
  const float* const rec0 = a.rec[0]; const float* const rec1 = a.rec[1];
  const bool has_scale = a.absmax != nullptr;
  auto tile_of = [&](int item) {
    const int k = two_pairs ? item >> 1 : item;
    return rev ? wg + (my_tiles - 1 - k) * nwg : wg + k * nwg;
  };

  // ---- issue the LDS-DMA of one item into its ring slot: wave w copies the 1-KiB fragments w, w + 8 of every plane, its
  // own copy of the scaled operand's record, and (narrow job) quarter w & 3 of the float32 B tile.  Everything goes
  // through LDS-DMA: with no register loads in the loop the only vmcnt waits are the counted ones below.
  auto issue = [&](int item) {
    const int t = tile_of(item), pi = two_pairs ? item & 1 : 0;
    const float* pa = (pi ? pa1 : pa0) + (size_t)t * (pi ? sa1 : sa0);
    const float* pb = (pi ? pb1 : pb0) + (size_t)t * (pi ? sb1 : sb0);
    unsigned char* slot = ring + (item % kRing) * kSlotAll;
    // (the planes of a block are contiguous in memory and in the slot: piece index 16 = the mid plane's first piece)
#pragma unroll
    for (int j = 0; j < 2 * R::kPlanes; ++j) {
      const int piece = wave + 8 * j;
      __builtin_amdgcn_global_load_lds((gvoid)(reinterpret_cast<const f32x4*>(pa) + piece * 64 + lane),
                                       SVS_LDS(void, slot + piece * 1024), 16, 0, 0);
      if (!narrow)
        __builtin_amdgcn_global_load_lds((gvoid)(reinterpret_cast<const f32x4*>(pb) + piece * 64 + lane),
                                         SVS_LDS(void, slot + kB + piece * 1024), 16, 0, 0);
    }
    if (narrow)
      __builtin_amdgcn_global_load_lds((gvoid)(reinterpret_cast<const f32x4*>(pb) + (wave & 3) * 64 + lane),
                                       SVS_LDS(void, slot + kB + (wave & 3) * 1024), 16, 0, 0);
    // scale record of the scaled operand: pair 0 scales A (abar-like), pair 1 B (u); applied to A either way
    if (has_scale)
      __builtin_amdgcn_global_load_lds((gvoid)((pi ? rec1 : rec0) + (size_t)t * 64 + lane),
                                       SVS_LDS(void, slot + kSlot + wave * 256), 4, 0, 0);
  };
  // ---- L2 prefetch of the item AFTER the one being copied (GP ring: 2 slots of 64 KiB fill the LDS, so only ONE item can be
  // in flight into LDS while one is multiplied -- 64 KiB per CU is less than HBM's latency-bandwidth product wants).  Every
  // thread reads 4 bytes of one 128-byte line of the item after next into a register nobody reads: the line comes into
  // the XCD's L2, and the LDS-DMA of that item, issued one iteration later, finds it there.  One extra vector-memory
  // operation per wave and item, issued BEHIND the item's copies (loads return in order: the counted wait below lets it
  // stay in flight).
  unsigned sink = 0;
  auto touch = [&](int item) {
    const int t = tile_of(item), pi = two_pairs ? item & 1 : 0;
    const Pair& p = a.p[pi];
    constexpr int kLines = R::kPlanes * (kPlane / 128);          // 128-byte lines per operand block
    const int nb = narrow ? 32 : kLines;
    const float* q = tid < kLines ? p.a + (size_t)t * p.stride_a + tid * 32
                                  : p.b + (size_t)t * p.stride_b + (tid - kLines) * 32;
    if (tid < kLines + nb) asm volatile("global_load_dword %0, %1, off" : "+v"(sink) : "v"(q) : "memory");
  };
  // number of vector-memory operations issue() makes per wave and item
  const int ops = (narrow ? 2 * R::kPlanes + 1 : 4 * R::kPlanes) + (has_scale ? 1 : 0);

  // ---- per-item set-up once the wave's own copies have landed: its factor table; (narrow job) the fp16 B image -- whose
  // float32 source quarters were copied by waves 0..3, hence after the barrier
  auto stage_factors = [&](int item) {
    unsigned char* slot = ring + (item % kRing) * kSlotAll;
    const int t = tile_of(item);
    const int live = n_valid - t * 32;
    float f = 1.0f;
    if (has_scale) {
      // s / s_p: the record is a power of two in [2^-107, 2^107] (PointScale::pow2_for); anything else (a block that
      // was never written) leaves the factor at 1
      float rec;
      lds_read32(rec, lds_addr(slot + kSlot + wave * 256 + 4 * wp));
      lds_wait();
      const unsigned eb = (__float_as_uint(rec) >> 23) & 0xff;
      if (eb >= 20 && eb <= 240) f = __builtin_fminf(s_grad * __uint_as_float((254u << 23) - __float_as_uint(rec)), 32768.0f);
    }
    if (wp >= live) f = 0.0f;
    // (inline assembly: a store hipcc can see is made to wait for every LDS-DMA in flight)
    // (the table is in the fragments' point order: maps::factor_pos)
    if (lane < 32) asm volatile("ds_write_b16 %0, %1" :: "v"(lds_addr(slot + kSlot + kRecBytes + wave * 64 + 2 * maps::factor_pos(wp))), "v"((_Float16)f) : "memory");
  };
  auto stage_narrow = [&](int item) {
    unsigned char* slot = ring + (item % kRing) * kSlotAll;
    if (tid < 256) {
      f32x4 v;
      lds_read128(v, lds_addr(slot + kB + tid * 16));
      lds_wait();
      f16x4 hi, mid;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const _Float16 h = (_Float16)v[j];
        hi[j] = h;
        mid[j] = (_Float16)(v[j] - (float)h);
      }
      *SVS_LDS(f16x4, slot + kB + kNarrowImg + wxoff) = hi;
      *SVS_LDS(f16x4, slot + kB + kNarrowImg + kExtraPiece + wxoff) = mid;
    }
  };

  const f16x2 one2 = {(_Float16)1.0f, (_Float16)1.0f};

  // ---- prologue: kAhead items in flight
  for (int i0 = 0; i0 < kAhead && i0 < n_items; ++i0) issue(i0);
  const bool touching = GP && ma.touch;
  bool touched = false;                  // a touch is the youngest outstanding operation of this wave
  if (touching && kAhead < n_items) { touch(kAhead); touched = true; }
  // ---- what a wave does for item `it` once its own copies of it have landed: its factor table.  The wait names how many
  // operations of later items (up to kAhead - 1 of them) may stay outstanding.  (Doing this for item + 1 in front of the last two
  // B tiles of item, so that the table's LDS round trip overlaps the other wave's MFMAs: measured equal or slower, 787-791
  // against 777-786 us alone -- the copy is barely ahead of the multiply phase and the early wait sometimes stalls.)
  auto pre_stage = [&](int it) {
    const int left = n_items - 1 - it;
    const int later = (left < kAhead - 1 ? left : kAhead - 1) * ops;        // 0, ops or 2 ops: 0, 3, 4, 5, 6, 8, 10 (GP: 0)
    if (later == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (later == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (later == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (later == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (later == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (later == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (touched) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");       // (GP: later == 0; the touch stays in flight)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_factors(it);
  };
  for (int item = 0; item < n_items; ++item) {
    const int pi = two_pairs ? item & 1 : 0;
    const bool p0 = pi == 0;
    // the item's own operations are the oldest outstanding ones of this wave; once every wave has waited for its own, everybody's
    // have landed behind the barrier -- which also says that every wave is done with the slot of item - 1, the one
    // item + kAhead is about to be copied into
    pre_stage(item);
    // (raw s_barrier: __syncthreads() carries a fence that hipcc lowers to vmcnt(0), which would also wait for the
    // next item's copies)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (narrow) {
      stage_narrow(item);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    auto issue_next = [&]() {
      if (item + kAhead < n_items) issue(item + kAhead);
      touched = false;
      if (touching && item + kAhead + 1 < n_items) { touch(item + kAhead + 1); touched = true; }
    };
    const unsigned la = lds_addr(ring + (item % kRing) * kSlotAll);
    const unsigned lb = la + kB;
    const unsigned ftab = la + kSlot + kRecBytes + wave * 64;
    const unsigned a_even = la + a_off + rd_even, a_odd = la + a_off + rd_odd;
    const unsigned b_even = lb + rd_even, b_odd = lb + rd_odd;
    const unsigned n_rd = lb + kNarrowImg + rx;
    const bool want_bias = has_db && p0;
    const bool two = narrow;             // only the narrow float32 tile is split into two pieces
    // The wave's A fragments (hi and mid pieces of its kRT row tiles) and their factors are requested together, the next item's
    // copies are issued behind the requests, and the fragments are waited for once: the item period is the multiply phase plus
    // what precedes it serially in every wave (section 3f of NOTES/r06.md).
    Frag fa[kRT], fam[kRT];
    f32x4 fraw;
    static_for<kRT>([&](auto oc) {
      constexpr int o = decltype(oc)::value;
      tr_issue<1024 * o>(fa[o], o & 1 ? a_odd : a_even);
      if (GP) tr_issue<kPlane + 1024 * o>(fam[o], o & 1 ? a_odd : a_even);
    });
    lds_read128(fraw, ftab + 16 * rg);   // the factors of the lane group's 8 points
    issue_next();        // (the next item's copies are issued while these reads are on their way)
    lds_wait();
    f16x8 ah[kRT], am[kRT];
#pragma unroll
    for (int o = 0; o < kRT; ++o) {
      ah[o] = frag_of(fa[o]) * __builtin_bit_cast(f16x8, fraw);
      am[o] = GP ? frag_of(fam[o]) * __builtin_bit_cast(f16x8, fraw) : ah[o];
      if (want_bias) {
        // row sums of A: the fragment holds 8 points of row lane & 15 (the other three lane groups hold the other 24)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f16x2 h2v = {ah[o][2 * j], ah[o][2 * j + 1]};
          bsum[o] = __builtin_amdgcn_fdot2(h2v, one2, bsum[o], false);
          if (GP) {
            const f16x2 m2v = {am[o][2 * j], am[o][2 * j + 1]};
            bsum[o] = __builtin_amdgcn_fdot2(m2v, one2, bsum[o], false);
          }
        }
      }
    }
    // the two waves of a SIMD cover each other's LDS latency: no software pipelining of the B fragments (requesting tile
    // i + 1's fragments before tile i's MFMAs, two register sets and a counted lgkmcnt: bit-identical, <= 1 % -- NOTES/r06.md 3f)
    static_for<kCT>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if (i < n_ct) {
        Frag fh, fm;
        if (!narrow) {
          tr_issue<1024 * i>(fh, i & 1 ? b_odd : b_even);
          if (GP) tr_issue<kPlane + 1024 * i>(fm, i & 1 ? b_odd : b_even);
        } else if constexpr (i < 2) {
          tr_issue<1024 * i>(fh, n_rd);
          tr_issue<kExtraPiece + 1024 * i>(fm, n_rd);
        }
        lds_wait();
        // every B fragment feeds all the wave's row tiles; per accumulator the products stay in the order hi mid, mid hi, hi hi
        const f16x8 bh = frag_of(fh), bm = frag_of(fm);
        if (two || GP) {
#pragma unroll
          for (int o = 0; o < kRT; ++o) acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[o], bm, acc[o][i], 0, 0, 0);
        }
        if (GP) {
#pragma unroll
          for (int o = 0; o < kRT; ++o) acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(am[o], bh, acc[o][i], 0, 0, 0);
        }
#pragma unroll
        for (int o = 0; o < kRT; ++o) acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[o], bh, acc[o][i], 0, 0, 0);
      }
    });
  }
  asm volatile("s_waitcnt vmcnt(0)" :: "v"(sink) : "memory");          // the last touch has returned; `sink` lived until here
  // flush: C[row = 4 (lane >> 4) + r][col = lane & 15] per tile, four 64-byte row segments per wave-instruction.  (Measured at
  // the rate of the two-segment shape a v_permlane16_swap of neighbouring column tiles gives: profiles/wgrad_shape.txt.)
  const int fcol = lane & 15;
  det::wait_turn(a.ticket, wg);
  static_for<kCT>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = a.col0 + 16 * i + fcol;
    if (i < n_ct && c < a.ldw) {
#pragma unroll
      for (int o = 0; o < kRT; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          atomicAdd(&a.dW[(size_t)(16 * (kRT * wave + o) + 4 * rg + r) * a.ldw + c], acc[o][i][r] * inv_s);
    }
  });
  if (a.db) {
#pragma unroll
    for (int o = 0; o < kRT; ++o) {
      float sum = bsum[o];
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      if (lane < 16) atomicAdd(&a.db[16 * (kRT * wave + o) + lane], sum * inv_s);
    }
  }
  det::pass_turn(a.ticket, wg);
}

}  // namespace h2

}  // namespace wgrad
}  // namespace svs

using namespace svs;
using namespace svs::wgrad;
namespace h2 = svs::wgrad::h2;

extern "C" {

// Weight gradients of several layers in one call.  Per job: dW[256][ldw] += sum_p A(p) B(p)^T over one or two
// operand pairs; db[256] += row sums of A of pair 0.  fp16x2: one launch for all jobs; float32: one launch per job.
int svs_wgrad_multi(const svs_wgrad_job* jobs, int n_jobs, int precision, void* hip_stream) {
  if (!jobs || n_jobs < 1) { set_error("svs_wgrad_multi: no jobs"); return SVS_EINVAL; }
  int n_expanded = 0;
  for (int j = 0; j < n_jobs; ++j) n_expanded += jobs[j].b_extra ? 2 : 1;
  if (n_expanded > h2::kMaxJobs) { set_error("svs_wgrad_multi: at most %d jobs (b_extra counts twice)", h2::kMaxJobs); return SVS_EINVAL; }
  for (int j = 0; j < n_jobs; ++j) {
    const svs_wgrad_job& q = jobs[j];
    if (!q.a0 || !q.b0 || !q.dW || q.n_points <= 0 || q.ldw < 256 || q.ldw > 288 || (q.b_extra && q.ldw < 288) || (q.a1 && !q.b1)) {
      set_error("svs_wgrad_multi: bad argument in job %d", j); return SVS_EINVAL;
    }
    if (mlp::is_h2(precision) && q.absmax && (!q.rec0 || (q.a1 && !q.rec1))) {
      set_error("svs_wgrad_multi: job %d has absmax but no scale records", j); return SVS_EINVAL;
    }
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (mlp::is_h2(precision)) {
    const bool gp = precision == mlp::kFmtF16x2;
    h2::MultiArgs ma;
    int n = 0;
    long long work[h2::kMaxJobs], total = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const svs_wgrad_job& q = jobs[j];
      h2::Job& J = ma.job[n];
      J.p[0] = Pair{q.a0, q.b0, (size_t)q.sa0, (size_t)q.sb0};
      J.rec[0] = q.rec0; J.rec[1] = q.rec1;
      J.n_pairs = 1;
      if (q.a1) { J.p[1] = Pair{q.a1, q.b1, (size_t)q.sa1, (size_t)q.sb1}; J.n_pairs = 2; }
      else { J.p[1] = J.p[0]; J.rec[1] = J.rec[0]; }
      J.n_tiles = (q.n_points + 31) / 32; J.n_valid_points = q.n_points;
      J.b_tiles = 8; J.col0 = 0; J.dW = q.dW; J.ldw = q.ldw; J.db = q.db; J.absmax = q.absmax;
      work[n] = (long long)J.n_tiles * J.n_pairs * 10;
      total += work[n++];
      if (q.b_extra) {
        // the 16 extra B rows (dW columns 256..271) as a narrow job of its own: same A, one 32-row B tile
        h2::Job& X = ma.job[n];
        X = J;
        X.p[0].b = q.b_extra; X.p[0].stride_b = (size_t)q.s_extra; X.n_pairs = 1;
        X.b_tiles = 1; X.col0 = 256; X.db = nullptr;
        // (a narrow item copies 36 of a wide item's 64 KiB and multiplies one B tile of eight, but an item's time is mostly
        // the latency of its copy: priced at 4 / 10 of a wide item, as until round 6, its workgroups were the radiance launch's
        // longest -- 0.33 ms alone; 5 ... 7: 0.29-0.30; 8, 10: 0.30-0.31 (profiles/r06_wgrad_what_bounds_it.txt))
        work[n] = (long long)X.n_tiles * 6;
        total += work[n++];
      }
    }
    ma.n_jobs = n;
    static const int touch_env = [] { const char* e = getenv("SVS_WGRAD_TOUCH"); return e ? atoi(e) : 0; }();
    ma.touch = touch_env;
    static const int reverse_env = [] { const char* e = getenv("SVS_WGRAD_REVERSE"); return e ? atoi(e) : 0; }();
    ma.reverse = reverse_env;
    // One workgroup per CU in total, at least one per job and no more than a job has tiles; the rest are handed out one at a
    // time to the job whose workgroups carry the most work (the launch lasts as long as its longest workgroup: with jobs of
    // very different sizes -- a step's two ray groups in one launch -- rounding each share on its own left a small job's
    // single workgroup with a third more tiles than anybody else)
    (void)total;
    const int n_wg_total = 256;
    int count[h2::kMaxJobs];
    int used = 0;
    for (int j = 0; j < n; ++j) { count[j] = 1; ++used; }
    while (used < n_wg_total) {
      int best = -1;
      double load = 0.0;
      for (int j = 0; j < n; ++j) {
        if (count[j] >= ma.job[j].n_tiles) continue;
        const double l = (double)work[j] / count[j];
        if (l > load) { load = l; best = j; }
      }
      if (best < 0) break;
      ++count[best]; ++used;
    }
    int begin = 0;
    for (int j = 0; j < n; ++j) {
      ma.job[j].wg_begin = begin; ma.job[j].wg_count = count[j];
      begin += count[j];
      ma.job[j].ticket = det::Ticket{nullptr, 0u, 0u};
    }
    if (deterministic()) {
      // jobs that add into the same columns of the same accumulator (the ray groups of a step) share a turn counter; their
      // workgroups take tickets in job order, then block order
      int owner[h2::kMaxJobs], n_owner = 0;
      for (int j = 0; j < n; ++j) {
        owner[j] = -1;
        for (int k = 0; k < j; ++k)
          if (ma.job[k].dW == ma.job[j].dW && ma.job[k].col0 == ma.job[j].col0) { owner[j] = owner[k]; break; }
        if (owner[j] < 0) owner[j] = n_owner++;
      }
      unsigned* turn = det::take_slots((unsigned)n_owner);
      if (!turn) { set_error("svs_wgrad_multi: no turn counters (deterministic mode)"); return SVS_EINVAL; }
      unsigned total[h2::kMaxJobs] = {0};
      for (int j = 0; j < n; ++j) { ma.job[j].ticket.turn = turn + owner[j]; ma.job[j].ticket.first = total[owner[j]]; total[owner[j]] += (unsigned)count[j]; }
      for (int j = 0; j < n; ++j) ma.job[j].ticket.total = total[owner[j]];
    }
    static hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(h2::wgrad_h2_multi_kernel<false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, h2::Ring<false>::kLdsBytes);
    static hipError_t ep = hipFuncSetAttribute(reinterpret_cast<const void*>(h2::wgrad_h2_multi_kernel<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, h2::Ring<true>::kLdsBytes);
    if (e != hipSuccess || ep != hipSuccess) {
      set_error("svs_wgrad_multi: hipFuncSetAttribute: %s", hipGetErrorString(e != hipSuccess ? e : ep)); return (int)(e != hipSuccess ? e : ep);
    }
    if (gp) h2::wgrad_h2_multi_kernel<true><<<begin, h2::kThreadsW, h2::Ring<true>::kLdsBytes, s>>>(ma);
    else h2::wgrad_h2_multi_kernel<false><<<begin, h2::kThreadsW, h2::Ring<false>::kLdsBytes, s>>>(ma);
    return check_launch("svs_wgrad_multi");
  }
  if (precision != mlp::kFmtF32) { set_error("svs_wgrad_multi: unknown precision %d", precision); return SVS_EINVAL; }
  for (int j = 0; j < n_jobs; ++j) {
    const svs_wgrad_job& q = jobs[j];
    Args a;
    a.p[0] = Pair{q.a0, q.b0, (size_t)q.sa0, (size_t)q.sb0};
    a.n_pairs = 1;
    if (q.a1) { a.p[1] = Pair{q.a1, q.b1, (size_t)q.sa1, (size_t)q.sb1}; a.n_pairs = 2; }
    a.n_tiles = (q.n_points + 31) / 32;
    a.n_valid_points = q.n_points;
    a.b_extra = q.b_extra; a.stride_extra = (size_t)q.s_extra;
    a.dW = q.dW; a.ldw = q.ldw; a.db = q.db;
    const int grid = a.n_tiles < 256 ? a.n_tiles : 256;
    a.ticket = det::Ticket{det::take_slots(1), 0u, (unsigned)grid};
    if (q.b_extra) {
      constexpr int lds = 2 * 32 * (260 + 292) * 4;
      static hipError_t e9 = hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_kernel<9>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e9 != hipSuccess) { set_error("svs_wgrad_multi: hipFuncSetAttribute: %s", hipGetErrorString(e9)); return (int)e9; }
      wgrad_kernel<9><<<grid, 256, lds, s>>>(a);
    } else {
      constexpr int lds = 2 * 32 * (260 + 260) * 4;
      static hipError_t e8 = hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_kernel<8>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e8 != hipSuccess) { set_error("svs_wgrad_multi: hipFuncSetAttribute: %s", hipGetErrorString(e8)); return (int)e8; }
      wgrad_kernel<8><<<grid, 256, lds, s>>>(a);
    }
    if (int rc = check_launch("svs_wgrad_multi")) return rc;
  }
  return SVS_OK;
}

// single job (see svs_wgrad_multi)
int svs_wgrad(const float* a0, const float* b0, long long sa0, long long sb0, const float* a1, const float* b1,
              long long sa1, long long sb1, const float* b_extra, long long s_extra, int n_points, int precision,
              const float* absmax, const float* rec0, const float* rec1, float* dW, int ldw, float* db, void* hip_stream) {
  svs_wgrad_job q{a0, b0, sa0, sb0, a1, b1, sa1, sb1, b_extra, s_extra, n_points, ldw, dW, db, absmax, rec0, rec1};
  return svs_wgrad_multi(&q, 1, precision, hip_stream);
}

}  // extern "C"
