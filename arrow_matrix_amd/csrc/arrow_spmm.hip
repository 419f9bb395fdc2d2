// arrow_spmm.hip — MI355X (gfx950, CDNA4) kernels for the arrow-SpMM hot path.
//
// Built from scratch for CDNA4; replaces the reference's cupy/cuSPARSE CSRMM
// calls (spcl/arrow-matrix arrow_slim_mpi.py:158-244) and host permutation
// gathers (arrow_dec_mpi.py:421-437,526-544). See include/arrow_spmm.h for
// the ABI contract.
//
// float32, float64 and bfloat16-feature SpMM share every kernel and the
// launch path: the code is written once over the element type, and Prec<T>
// below holds the little that differs. A change to the shared body is checked against the build
// before it with tools/isa_diff.py (gfx950 assembly, kernel by kernel).
//
// Kernel design (CSR x tall-skinny dense, k = 1..128 typical; figures are
// for fp32, a float64 lane carries the same 16 bytes as double2):
//   * The path is HBM-bandwidth-bound (AI ~= 2.3 flop/byte), not a dense
//     contraction -> no MFMA. The levers are coalescing and load balance.
//   * k is mapped across lanes of a 64-wide wavefront in GROUP-lane
//     "row groups", each lane loading VEC consecutive floats of an X row
//     (float4 when k % 4 == 0) -> one fully-coalesced 64..512 B read per
//     touched X row, and coalesced C writes.
//   * Load balance on power-law rows (the first block-row A_0i holds the
//     hub vertices): rows are pre-split at upload time into work items of
//     at most SEG_NNZ nonzeros; split rows accumulate into C with
//     global fp32 atomics, whole rows write directly. Every row gets an
//     item, so beta=0 also zeroes empty rows.
//   * A's (col, val) stream is read once per item by all lanes of the
//     group (same-address broadcast within the wave's transaction).
//   * Work items are consumed either by a grid-stride loop (small
//     structures) or by the per-XCD queue scheduler (GROUP >= 4 and
//     >= 32M nnz by default): 8 contiguous nnz-balanced item segments
//     drained via per-XCD atomic chunk counters so each XCD walks one
//     tight X window in order (measured +54 % at k=128). Grabs are per
//     WORKGROUP at GROUP >= 8 (spmm_kernel_q) and per WAVE at GROUP < 8
//     (spmm_kernel_qw — no __syncthreads rendezvous; k=16 measured
//     +15 % over grid-stride, profiles/r02_ab2_sweep.log).

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/arrow_spmm.h"

#define ARROW_ABI_VERSION 1007  // operator scaling (arrow_csr_sums, arrow_csr_scale)

namespace {

thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));            \
      return -1;                                                               \
    }                                                                          \
  } while (0)

constexpr int SEG_NNZ = 2048;     // max nonzeros per work item
constexpr int BLOCK_THREADS = 256;

struct CsrBlock {
  int64_t rows = 0, cols = 0, nnz = 0;
  // (col, val) packed 8-byte pairs (device, nnz). col < 0 encodes an index
  // into the SECOND feature matrix of arrow_spmm_dual: col = -(idx+1)
  // (the fused diagonal+first-block-column layout).
  int2 *pairs = nullptr;
  // precision tag, fixed at creation: 32 (pairs above) or 64 (the split
  // arrays below, 12 B/nnz; pairs stays null)
  int dtype = 32;
  int32_t *cols64 = nullptr;
  double *vals64 = nullptr;
  // work items (device): row (bit31 = atomic), [begin, end) into pairs
  int32_t *item_row = nullptr;
  int32_t *item_begin = nullptr;
  int32_t *item_end = nullptr;
  int64_t n_items = 0;
  // device: [n_split_rows, then the split rows' output rows in ascending
  // order]. split_rows points at the rows (pre-zeroed at beta=0 by the fp32
  // and f64 paths); the bf16 kernels search them for a row's scratch slot.
  int32_t *split_tab = nullptr;
  int32_t *split_rows = nullptr;
  int64_t n_split_rows = 0;
  // bf16 features only: fp32 partial sums of the split rows, n_split_rows x
  // scratch_k floats, all zero between launches. Allocated on the first
  // arrow_spmm_bf16 call that needs it and only ever grown (never inside a
  // launch that may be under stream capture: warm up first).
  float *bf16_scratch = nullptr;
  int64_t scratch_k = 0;
  // XCD-contiguous item remap for this structure (uniform banded rows only:
  // on hub-heavy structures it serialises the heavy head onto one XCD)
  int xcd_remap = 0;
  // per-XCD queue scheduler: -1 follow ARROW_QUEUE env, 0 off, 1 on
  int queue_mode = -1;
  int64_t *qseg = nullptr;  // device, 9 nnz-balanced item-segment bounds
  int32_t *qctr = nullptr;  // device, 8 chunk counters padded 32 ints apart
  int q_blocks = 0;         // per-structure grid override (0 = ARROW_Q_BLOCKS)
};

std::unordered_map<int64_t, CsrBlock> g_blocks;
int64_t g_next_handle = 1;

// ---------------------------------------------------------------------------
// SpMM kernel, float and double.  GROUP lanes x VEC elements cover
// min(k, GROUP*VEC) columns; wider k is handled by a column-offset loop over
// launches (col_off). A lane covers at most 16 bytes of an X row: float4, or
// double2 (the same bytes), or 8 bf16. Accumulation is fma in T (in float
// for bf16 features); split rows add with the hardware global atomic of T
// (bf16: of float, into the structure's scratch).
// The per-item body is shared by the three schedulers below (grid-stride,
// block-grab and wave-grab per-XCD queue) — spmm_process_item computes one
// work item end to end.
// ---------------------------------------------------------------------------

// What differs between the two precisions, and nothing else. The A stream
// reaches the kernels as plain `const A *__restrict__...` parameters (the
// pack A... is {int2} for float, {int32_t, double} for double), so each
// precision keeps its own kernarg layout and its restrict information.
//   float : (col, val) packed 8-byte pairs, one 8-B load per lane per GROUP
//           nonzeros; the value is one shuffle.
//   double: SPLIT arrays int32 cols[] + double vals[] (12 B/nnz; a padded
//           16-byte record would waste a third of the A stream), a
//           coalesced 4-B and a coalesced 8-B load per GROUP nonzeros; the
//           64-bit value travels as two 32-bit shuffles.
//   bf16  : T = uint16_t, the raw bits of a bfloat16 FEATURE (X and C). A is
//           the float stream unchanged and every product and partial sum is
//           fp32: a lane loads 8 bf16 (16 bytes), widens each by a 16-bit
//           shift, accumulates 8 floats with fmaf and rounds once, on the
//           way out (plain cast: round-to-nearest-even, NaN stays NaN).
//           Split rows add their fp32 partials into the structure's scratch
//           and spmm_finalise_bf16 rounds them once (a bf16 atomic would
//           round the running sum at every add).
// Per precision: Acc is the accumulator, XV<VEC> a lane's VEC stored
// elements, unpack / pack convert between the two (the identity for float
// and double), split_add is what a split-row item does with its partials.
template <typename T> struct Prec;

// 8 bf16 in 16 bytes <-> 8 floats. Element 2i is the low half of word i.
struct Float8 {
  float e[8];
  __device__ __forceinline__ float operator[](int j) const { return e[j]; }
  __device__ __forceinline__ float &operator[](int j) { return e[j]; }
};

__device__ __forceinline__ Float8 bf16x8_unpack(const uint4 &w) {
  Float8 f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f.e[2 * i] = __uint_as_float(w[i] << 16);
    f.e[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
  return f;
}

__device__ __forceinline__ uint4 bf16x8_pack(const float *s) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  uint4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 v = {s[2 * i], s[2 * i + 1]};
    w[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  }
  return w;
}

// unpack / pack / split_add of a precision whose stored element is its
// accumulator (float, double)
template <typename T> struct PrecSame {
  using Acc = T;
  using Word = T;  // element of XV and of the non-temporal store vector
  template <int VEC> static constexpr int WORDS = VEC;
  template <int VEC> using XV = HIP_vector_type<T, VEC>;
  template <int VEC>
  __device__ static __forceinline__ const XV<VEC> &unpack(const XV<VEC> &x) {
    return x;
  }
  template <int VEC>
  __device__ static __forceinline__ XV<VEC> pack(const T *s) {
    XV<VEC> o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = s[j];
    return o;
  }
  template <int VEC>
  __device__ static __forceinline__ const XV<VEC> &pack(const XV<VEC> &x) {
    return x;
  }
  // the hardware global atomic of T, straight into C
  template <int VEC, typename... A>
  __device__ static __forceinline__ void split_add(T *cr, int32_t, int64_t,
                                                   int64_t, const T *acc,
                                                   const A *...) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) atomicAdd(cr + j, acc[j]);
  }
};

template <> struct Prec<float> : PrecSame<float> {
  static constexpr int dtype = 32;  // of the structure the entry points take
  static constexpr const char *suffix = "";
  static constexpr const char *name = "float32";
  using Staged = int2;  // one staged nonzero per lane
  // nontemporal A-stream load (each pair is read once by one wave): the
  // builtin wants a native vector type, HIP's int2 is a class
  __device__ static __forceinline__ Staged load(int nt, int32_t idx,
                                                const int2 *pairs) {
    typedef int nt_int2 __attribute__((ext_vector_type(2)));
    if (nt) {
      const nt_int2 raw = __builtin_nontemporal_load(
          reinterpret_cast<const nt_int2 *>(pairs + idx));
      return int2{raw.x, raw.y};
    }
    return pairs[idx];
  }
  template <int GROUP>
  __device__ static __forceinline__ int32_t col(const Staged &mine, int u) {
    return __shfl(mine.x, u, GROUP);
  }
  template <int GROUP>
  __device__ static __forceinline__ float val(const Staged &mine, int u) {
    return __int_as_float(__shfl(mine.y, u, GROUP));
  }
  __device__ static __forceinline__ float mad(float a, float b, float c) {
    return fmaf(a, b, c);
  }
  // a lane's own staged nonzero, no shuffle (the operator passes below), and
  // the write-back of a rescaled value: the whole pair, one coalesced 8 B
  __device__ static __forceinline__ int32_t own_col(const Staged &mine) {
    return mine.x;
  }
  __device__ static __forceinline__ float own_val(const Staged &mine) {
    return __int_as_float(mine.y);
  }
  __device__ static __forceinline__ void store_val(int32_t idx, int32_t col,
                                                   float v, int2 *pairs) {
    pairs[idx] = int2{col, __float_as_int(v)};
  }
  template <typename F> static int with_stream(const CsrBlock &blk, F f) {
    return f(blk.pairs);
  }
};

template <> struct Prec<double> : PrecSame<double> {
  static constexpr int dtype = 64;
  static constexpr const char *suffix = "_f64";
  static constexpr const char *name = "float64";
  struct Staged { int32_t c, lo, hi; };
  __device__ static __forceinline__ Staged load(int nt, int32_t idx,
                                                const int32_t *cols,
                                                const double *vals) {
    int32_t c;
    double v;
    if (nt) {
      c = __builtin_nontemporal_load(cols + idx);
      v = __builtin_nontemporal_load(vals + idx);
    } else {
      c = cols[idx];
      v = vals[idx];
    }
    return Staged{c, __double2loint(v), __double2hiint(v)};
  }
  template <int GROUP>
  __device__ static __forceinline__ int32_t col(const Staged &mine, int u) {
    return __shfl(mine.c, u, GROUP);
  }
  template <int GROUP>
  __device__ static __forceinline__ double val(const Staged &mine, int u) {
    return __hiloint2double(__shfl(mine.hi, u, GROUP),
                            __shfl(mine.lo, u, GROUP));
  }
  __device__ static __forceinline__ double mad(double a, double b, double c) {
    return fma(a, b, c);
  }
  __device__ static __forceinline__ int32_t own_col(const Staged &mine) {
    return mine.c;
  }
  __device__ static __forceinline__ double own_val(const Staged &mine) {
    return __hiloint2double(mine.hi, mine.lo);
  }
  __device__ static __forceinline__ void store_val(int32_t idx, int32_t,
                                                   double v, int32_t *,
                                                   double *vals) {
    vals[idx] = v;
  }
  template <typename F> static int with_stream(const CsrBlock &blk, F f) {
    return f(blk.cols64, blk.vals64);
  }
};

// bf16 features over the float A stream. The kernels' pointer pack carries,
// after the pairs, the split-row table and the fp32 scratch, so the float
// and double kernels keep their parameter lists.
template <> struct Prec<uint16_t> : Prec<float> {
  static constexpr const char *suffix = "_bf16";
  static constexpr const char *name = "bfloat16";
  using Acc = float;
  using Word = unsigned;
  template <int VEC> static constexpr int WORDS = VEC / 2;
  template <int VEC> using XV = uint4;  // VEC is 8
  __device__ static __forceinline__ Staged load(int nt, int32_t idx,
                                                const int2 *pairs,
                                                const int32_t *,
                                                const float *) {
    return Prec<float>::load(nt, idx, pairs);
  }
  template <int VEC>
  __device__ static __forceinline__ Float8 unpack(const uint4 &x) {
    return bf16x8_unpack(x);
  }
  template <int VEC>
  __device__ static __forceinline__ uint4 pack(const float *s) {
    return bf16x8_pack(s);
  }
  template <int VEC>
  __device__ static __forceinline__ uint4 pack(const Float8 &x) {
    return bf16x8_pack(x.e);
  }
  // tab[0] = n >= 1 (the structure has a split item), tab[1..n] ascending
  // and holding `row`: its index is the scratch slot. Clamped, so that even
  // a row that were missing could not index outside the scratch.
  __device__ static __forceinline__ int32_t split_slot(int32_t row,
                                                       const int32_t *tab) {
    const int32_t n = tab[0];
    int32_t lo = 0, hi = n;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (tab[1 + mid] < row) lo = mid + 1;
      else                    hi = mid;
    }
    return lo < n ? lo : n - 1;
  }
  template <int VEC>
  __device__ static __forceinline__ void split_add(uint16_t *, int32_t row,
                                                   int64_t k, int64_t col0,
                                                   const float *acc,
                                                   const int2 *,
                                                   const int32_t *tab,
                                                   const float *scratch) {
    float *sr = const_cast<float *>(scratch) +
                (int64_t)split_slot(row, tab) * k + col0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) atomicAdd(sr + j, acc[j]);
  }
  template <typename F> static int with_stream(const CsrBlock &blk, F f) {
    return f(blk.pairs, (const int32_t *)blk.split_tab,
             (const float *)blk.bf16_scratch);
  }
};

// What an item does with its finished sums on the way out, chosen at compile
// time (EP). NoEpilogue is the plain C (+)= A@X and carries nothing: the
// plain kernels are the instructions they were before the epilogue existed
// (profiles/isa_affine_parent_vs_branch.txt). AffineEpilogue is the fused
// affine step C = alpha * (A@X) + gamma * R (+ C): alpha and gamma are
// applied in the accumulator type, R is indexed like C (by output row) and
// is null when gamma == 0, in which case it is never dereferenced.
struct NoEpilogue {};
template <typename T> struct AffineEpilogue {
  const T *R;
  typename Prec<T>::Acc alpha, gamma;
};
// AffineNormEpilogue is the affine step that also measures it: every
// non-split row adds sum (c - d)^2 and sum c^2 over its stored values c and
// the stored values d of D[row] (indexed like R; null means d = 0). c - d is
// formed in the accumulator type, squares and sums are double. Beta is 0. The
// kernel argument is AffineNormEpilogue; the items see AffineNormLane, which
// adds the thread's two running sums (they live across all of its items and
// leave through norm_block_reduce at kernel exit).
template <typename T> struct AffineNormEpilogue {
  const T *R;
  typename Prec<T>::Acc alpha, gamma;
  const T *D;
  double *acc;  // device, two doubles, added into
};
template <typename T> struct AffineNormLane : AffineNormEpilogue<T> {
  double *sums;  // the thread's own {sum (c - d)^2, sum c^2}
};

// sums[0] += sum (c - d)^2, sums[1] += sum c^2 over N stored values
template <typename Acc, int N, typename CV, typename DV>
__device__ __forceinline__ void norm_add(double *sums, const CV &c,
                                         const DV &d) {
  // each square is rounded to double, then added: with d = 0 a thread's two
  // sums take the same terms in the same order and stay equal bit for bit (a
  // square fused into one sum's add and not the other's would part them).
  // The workgroups' atomics land in an order of their own per accumulator,
  // so the totals are equal only where the sums are exact.
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const Acc diff = Acc(c[j]) - Acc(d[j]);
    sums[0] += (double)diff * (double)diff;
    sums[1] += (double)c[j] * (double)c[j];
  }
}

// The exit of every kernel that measures: all 256 threads of the workgroup
// arrive here (no path returns early), the waves reduce by shuffle, the
// workgroup through LDS, and thread 0 adds the two totals with the hardware
// float64 atomic.
__device__ __forceinline__ void norm_block_reduce(double s0, double s1,
                                                  double *acc) {
  __shared__ double part[2][BLOCK_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off, 64);
    s1 += __shfl_down(s1, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = s0;
    part[1][threadIdx.x >> 6] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK_THREADS / 64; ++w) {
      s0 += part[0][w];
      s1 += part[1][w];
    }
    atomicAdd(acc, s0);
    atomicAdd(acc + 1, s1);
  }
}

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename EP,
          typename... A>
__device__ __forceinline__ void spmm_process_item(
    int32_t row_raw, int32_t b, int32_t e, const T *__restrict__ X0,
    const T *__restrict__ X1, T *__restrict__ C, int64_t k, int64_t col0,
    bool active, int lane_in_group, int nt_mode, EP ep,
    const A *__restrict__... a) {
  constexpr bool AFFINE = !std::is_same_v<EP, NoEpilogue>;
  constexpr bool NORM = std::is_same_v<EP, AffineNormLane<T>>;
  static_assert(!NORM || BETA == 0, "a launch that measures finishes its rows");
  using P = Prec<T>;
  using Staged = typename P::Staged;
  using Acc = typename P::Acc;  // products and partial sums
  using XV = typename P::template XV<VEC>;  // a lane's VEC elements of a row
  // a lane covers 16 bytes of storage (float4 / double2 / 8 bf16): the
  // widest load, the batched consume4 / consume8 and the vector write-back
  // are for this layout only
  constexpr bool LANE16 = VEC * sizeof(T) == 16;

  const int32_t row = row_raw & 0x7fffffff;
  const bool is_split = row_raw < 0;

  Acc acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = Acc(0);

  // Stage GROUP nonzeros cooperatively (ONE coalesced record load per lane
  // per GROUP nonzeros), then broadcast them across the group with wave
  // shuffles — the A stream costs 1/GROUP memory instructions per nonzero
  // instead of 2.
  auto xaddr = [&](const Staged &mine, int u) {
    const int32_t c = P::template col<GROUP>(mine, u);
    return (c < 0 ? X1 + (int64_t)(-c - 1) * k : X0 + (int64_t)c * k) + col0;
  };
  auto val = [&](const Staged &mine, int u) {
    return P::template val<GROUP>(mine, u);
  };
  // acc += v * x, lane element by lane element
  auto axpy = [&](Acc v, const XV &xs) {
    const auto &x = P::template unpack<VEC>(xs);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = P::mad(v, x[j], acc[j]);
  };
  auto consume = [&](const Staged &mine, int u) {
    const T *xr = xaddr(mine, u);
    const Acc v = val(mine, u);
    if (active) {
      if constexpr (VEC > 1) {
        axpy(v, *reinterpret_cast<const XV *>(xr));
      } else {
        acc[0] = P::mad(v, xr[0], acc[0]);
      }
    }
  };
  // 4 entries at a time with the four X-row loads issued back to back
  // BEFORE any use: the rolled one-at-a-time loop stalls on each load's
  // s_waitcnt before the next can issue (in-order issue), which makes
  // short power-law rows latency-bound.
  auto consume4 = [&](const Staged &mine, int u) {
    if constexpr (LANE16) {
      const T *p0 = xaddr(mine, u + 0);
      const T *p1 = xaddr(mine, u + 1);
      const T *p2 = xaddr(mine, u + 2);
      const T *p3 = xaddr(mine, u + 3);
      const Acc v0 = val(mine, u + 0), v1 = val(mine, u + 1);
      const Acc v2 = val(mine, u + 2), v3 = val(mine, u + 3);
      if (active) {
        const XV a0 = *reinterpret_cast<const XV *>(p0);
        const XV a1 = *reinterpret_cast<const XV *>(p1);
        const XV a2 = *reinterpret_cast<const XV *>(p2);
        const XV a3 = *reinterpret_cast<const XV *>(p3);
        axpy(v0, a0); axpy(v1, a1); axpy(v2, a2); axpy(v3, a3);
      }
    } else {
      consume(mine, u); consume(mine, u + 1);
      consume(mine, u + 2); consume(mine, u + 3);
    }
  };
  // 8 loads in flight: a deg-8 power-law row issues its entire X-row
  // load set before any use (the 4-deep batch still serialises pairs of
  // batches on in-order issue)
  auto consume8 = [&](const Staged &mine, int u) {
    if constexpr (LANE16 && GROUP >= 8) {
      const T *p[8];
      Acc v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = xaddr(mine, u + j);
        v[j] = val(mine, u + j);
      }
      if (active) {
        XV x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const XV *>(p[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) axpy(v[j], x[j]);
      }
    } else {
      consume4(mine, u);
      consume4(mine, u + 4);
    }
  };
  int32_t base = b;
  for (; base + GROUP <= e; base += GROUP) {  // full chunks
    const Staged mine = P::load(nt_mode, base + lane_in_group, a...);
    if constexpr (GROUP >= 8) {
#pragma unroll
      for (int u = 0; u < GROUP; u += 8) consume8(mine, u);
    } else if constexpr (GROUP >= 4) {
#pragma unroll
      for (int u = 0; u < GROUP; u += 4) consume4(mine, u);
    } else {
#pragma unroll
      for (int u = 0; u < GROUP; ++u) consume(mine, u);
    }
  }
  if (base < e) {  // remainder (< GROUP entries), cached loads
    const int32_t t = base + lane_in_group;
    const Staged mine = (t < e) ? P::load(0, t, a...) : Staged{};
    const int cnt = e - base;
    int u = 0;
    if constexpr (GROUP >= 8) {
      for (; u + 8 <= cnt; u += 8) consume8(mine, u);
    }
    for (; u + 4 <= cnt; u += 4) consume4(mine, u);
    for (; u < cnt; ++u) consume(mine, u);
  }

  if (active) {
    T *cr = C + (int64_t)row * k + col0;
    if (is_split) {
      // affine: the pre-launch pass put gamma * R (+ C) into the row and the
      // items add alpha * partial. bf16 partials go to the scratch unscaled;
      // spmm_finalise_affine_bf16 applies alpha and gamma * R once.
      if constexpr (AFFINE && sizeof(T) != 2) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] *= ep.alpha;
      }
      P::template split_add<VEC>(cr, row, k, col0, acc, a...);
    } else if constexpr (AFFINE) {
      // alpha * acc + gamma * r (+ old), one store. The lane that owns 16
      // bytes of C[row] loads the same 16 bytes of R[row] (cached: R is
      // reused every step); `active` guards both alike.
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] *= ep.alpha;
      if constexpr (LANE16) {
        if (ep.R) {
          const XV rv =
              *reinterpret_cast<const XV *>(ep.R + (int64_t)row * k + col0);
          const auto &r = P::template unpack<VEC>(rv);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = P::mad(ep.gamma, r[j], acc[j]);
        }
        if constexpr (BETA == 1) {
          const auto &old = P::template unpack<VEC>(*reinterpret_cast<XV *>(cr));
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] += old[j];
          *reinterpret_cast<XV *>(cr) = P::template pack<VEC>(acc);
        } else {
          const XV packed = P::template pack<VEC>(acc);
          if constexpr (NORM) {
            // the value as stored (bf16: unpack what was packed) against the
            // same 16 bytes of D[row]
            const XV dv = ep.D ? *reinterpret_cast<const XV *>(
                                     ep.D + (int64_t)row * k + col0)
                               : XV{};
            norm_add<Acc, VEC>(ep.sums, P::template unpack<VEC>(packed),
                               P::template unpack<VEC>(dv));
          }
          if (nt_mode) {
            constexpr int WORDS = P::template WORDS<VEC>;
            typedef typename P::Word nt_vec
                __attribute__((ext_vector_type(WORDS)));
            nt_vec outv;
#pragma unroll
            for (int j = 0; j < WORDS; ++j) outv[j] = packed[j];
            __builtin_nontemporal_store(outv, reinterpret_cast<nt_vec *>(cr));
          } else {
            *reinterpret_cast<XV *>(cr) = packed;
          }
        }
      } else {
        const T *rr = ep.R ? ep.R + (int64_t)row * k + col0 : nullptr;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          Acc o = acc[j];
          if (rr) o = P::mad(ep.gamma, rr[j], o);
          if constexpr (BETA == 1) o += cr[j];
          cr[j] = o;
          if constexpr (NORM) {
            const Acc d = ep.D ? ep.D[(int64_t)row * k + col0 + j] : Acc(0);
            norm_add<Acc, 1>(ep.sums, &o, &d);
          }
        }
      }
    } else if constexpr (BETA == 1) {
      if constexpr (LANE16) {
        auto old = P::template unpack<VEC>(*reinterpret_cast<XV *>(cr));
#pragma unroll
        for (int j = 0; j < VEC; ++j) old[j] += acc[j];
        *reinterpret_cast<XV *>(cr) = P::template pack<VEC>(old);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) cr[j] += acc[j];
      }
    } else {
      if constexpr (LANE16) {
        const XV packed = P::template pack<VEC>(acc);
        if (nt_mode) {
          constexpr int WORDS = P::template WORDS<VEC>;
          typedef typename P::Word nt_vec
              __attribute__((ext_vector_type(WORDS)));
          nt_vec outv;
#pragma unroll
          for (int j = 0; j < WORDS; ++j) outv[j] = packed[j];
          __builtin_nontemporal_store(outv, reinterpret_cast<nt_vec *>(cr));
        } else {
          *reinterpret_cast<XV *>(cr) = packed;
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) cr[j] = acc[j];
      }
    }
  }
}

// Items first, first + step, ... below end, one per row group: the loop all
// three schedulers run over their share of the work items.
// Software prefetch of the NEXT item's metadata: without it every ~8-nnz
// item pays a 3-deep dependent load chain (meta -> A stream -> X row) that
// dominates short power-law rows.
template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename EP,
          typename... A>
__device__ __forceinline__ void spmm_process_items(
    int64_t item, int64_t end, int64_t step, const int32_t *item_row,
    const int32_t *item_begin, const int32_t *item_end, const T *X0,
    const T *X1, T *C, int64_t k, int64_t col0, bool active,
    int lane_in_group, int nt_mode, EP ep, const A *... a) {
  int32_t next_row = 0, next_b = 0, next_e = 0;
  if (item < end) {
    next_row = __builtin_nontemporal_load(&item_row[item]);
    next_b = __builtin_nontemporal_load(&item_begin[item]);
    next_e = __builtin_nontemporal_load(&item_end[item]);
  }
  for (; item < end; item += step) {
    const int32_t row_raw = next_row;
    const int32_t b = next_b;
    const int32_t e = next_e;
    const int64_t nxt = item + step;
    if (nxt < end) {
      next_row = __builtin_nontemporal_load(&item_row[nxt]);
      next_b = __builtin_nontemporal_load(&item_begin[nxt]);
      next_e = __builtin_nontemporal_load(&item_end[nxt]);
    }
    spmm_process_item<T, VEC, GROUP, BETA, GUARD, EP>(
        row_raw, b, e, X0, X1, C, k, col0, active, lane_in_group, nt_mode, ep,
        a...);
  }
}

// Each scheduler has two entry symbols: the plain kernel (its parameter list,
// name and body are what they always were) and the _affine kernel, which
// takes the epilogue as one more argument. The epilogue is not a parameter of
// the plain kernels because even an empty struct takes a byte of the
// kernel-argument block, and their body is shared as TEXT (the *_BODY macros,
// with the epilogue expression as argument) rather than through one more
// inlined function, which was tried and moved instructions in all 504 plain
// kernels: they are to stay what they were, descriptor included.
#define SPMM_GRID_BODY(EPILOGUE)                                              \
  constexpr int GROUPS_PER_BLOCK = BLOCK_THREADS / GROUP;                     \
  const int lane_in_group = threadIdx.x % GROUP;                              \
  const int group_in_block = threadIdx.x / GROUP;                             \
  const int64_t col0 = col_off + (int64_t)lane_in_group * VEC;                \
  const bool active = !GUARD || (col0 < k);                                   \
                                                                              \
  /* XCD-aware workgroup remap (performance only): the dispatcher places     \
     block b on XCD b%8, so remap block ids to give each XCD a CONTIGUOUS    \
     range of work items: consecutive rows of a banded block then share the  \
     XCD's private L2 window instead of interleaving across all 8 L2s.       \
     Bijective form (cdna_hip_programming.md, XCD swizzle). */               \
  int wg = blockIdx.x;                                                        \
  if (xcd_remap) {                                                            \
    const int nwg = gridDim.x;                                                \
    const int q = nwg / 8, rm = nwg % 8;                                      \
    const int xcd = blockIdx.x % 8, pos = blockIdx.x / 8;                     \
    wg = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + pos;    \
  }                                                                           \
                                                                              \
  spmm_process_items<T, VEC, GROUP, BETA, GUARD>(                             \
      (int64_t)wg * GROUPS_PER_BLOCK + group_in_block, n_items,               \
      (int64_t)gridDim.x * GROUPS_PER_BLOCK, item_row, item_begin, item_end,  \
      X0, X1, C, k, col0, active, lane_in_group, nt_mode, EPILOGUE, a...)

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end, int64_t n_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int xcd_remap,
    int nt_mode) {
  SPMM_GRID_BODY(NoEpilogue{});
}

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_affine(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end, int64_t n_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int xcd_remap,
    int nt_mode, AffineEpilogue<T> ep) {
  SPMM_GRID_BODY(ep);
}

// The _affine_norm kernels: the same body once more, with the thread's two
// sums behind the epilogue and the workgroup's reduction after the loop.
template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_affine_norm(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end, int64_t n_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int xcd_remap,
    int nt_mode, AffineNormEpilogue<T> ep) {
  double sums[2] = {0.0, 0.0};
  SPMM_GRID_BODY((AffineNormLane<T>{ep, sums}));
  norm_block_reduce(sums[0], sums[1], ep.acc);
}

// Per-XCD queue scheduler. The static grid-stride schedule above interleaves
// consecutive work items across all 8 XCDs and lets workgroups DRIFT apart
// over millions of items, so the ~10 consumers of each 512-B X row (rows
// within ±band) hit different L2s at different times — measured 3.2x X
// re-fetch, 16 % L2 hit (profiles/r01_pmc_sq_tcc_20M.txt). Here items are
// split into 8 CONTIGUOUS nnz-balanced row segments; each workgroup drains
// the segment of the XCD it actually runs on (HW_REG_XCC_ID, speed-only)
// via an atomic chunk counter, so every XCD walks one tight row window in
// order: consumers of an X row share one private L2, and the in-flight
// window stays a few MB. Workgroups that exhaust their queue steal from the
// next (placement-independent correctness; the register read is only a
// locality hint — cdna_hip_programming.md §Guideline 16).
__device__ __forceinline__ unsigned arrow_xcc_id() {
  // s_getreg_b32 HW_REG_XCC_ID: reg 20, offset 0, size 4 (gfx950)
  return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);
}

#define SPMM_Q_BODY(EPILOGUE)                                                 \
  constexpr int GROUPS_PER_BLOCK = BLOCK_THREADS / GROUP;                     \
  const int lane_in_group = threadIdx.x % GROUP;                              \
  const int group_in_block = threadIdx.x / GROUP;                             \
  const int64_t col0 = col_off + (int64_t)lane_in_group * VEC;                \
  const bool active = !GUARD || (col0 < k);                                   \
  __shared__ int64_t s_base;                                                  \
                                                                              \
  const unsigned q0 = arrow_xcc_id() & 7;                                     \
  for (unsigned qi = 0; qi < 8; ++qi) {                                       \
    const unsigned q = (q0 + qi) & 7;                                         \
    const int64_t lo = qseg[q], hi = qseg[q + 1];                             \
    if (lo >= hi) continue;                                                   \
    for (;;) {                                                                \
      __syncthreads();                                                        \
      if (threadIdx.x == 0) {                                                 \
        s_base = lo + (int64_t)atomicAdd(&qctr[q * 32], chunk_items);         \
      }                                                                       \
      __syncthreads();                                                        \
      const int64_t base = s_base;                                            \
      if (base >= hi) break;                                                  \
      const int64_t end = base + chunk_items < hi ? base + chunk_items : hi;  \
      spmm_process_items<T, VEC, GROUP, BETA, GUARD>(                         \
          base + group_in_block, end, GROUPS_PER_BLOCK, item_row, item_begin, \
          item_end, X0, X1, C, k, col0, active, lane_in_group, nt_mode,       \
          EPILOGUE, a...);                                                    \
    }                                                                         \
  }

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_q(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg,  // 9 segment bounds (items)
    int32_t *__restrict__ qctr,       // 8 counters, padded 32 ints apart
    int chunk_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode) {
  SPMM_Q_BODY(NoEpilogue{})
}

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_q_affine(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg, int32_t *__restrict__ qctr,
    int chunk_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode,
    AffineEpilogue<T> ep) {
  SPMM_Q_BODY(ep)
}

// A workgroup that found every queue dry still falls through to the
// reduction: the body has no return.
template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_q_affine_norm(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg, int32_t *__restrict__ qctr,
    int chunk_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode,
    AffineNormEpilogue<T> ep) {
  double sums[2] = {0.0, 0.0};
  SPMM_Q_BODY((AffineNormLane<T>{ep, sums}))
  norm_block_reduce(sums[0], sums[1], ep.acc);
}

// Per-WAVE queue grab variant of spmm_kernel_q: each 64-lane wave pulls its
// own chunk from the XCD's counter (lane-0 atomicAdd broadcast by wave
// shuffle) — no __syncthreads per grab. Removes the whole-block rendezvous
// that made queues lose at small GROUP (k=16: 16 groups per wave stall on
// the slowest group of all 4 waves), at the cost of 4x the atomic rate
// (fine: per-XCD counters, dequeue ~0.25-1.1 us uncontended and these are
// thousands of grabs per segment, MI355X_MICROARCH.md §dequeue).
#define SPMM_QW_BODY(EPILOGUE)                                                \
  constexpr int GROUPS_PER_WAVE = 64 / GROUP;                                 \
  const int lane = threadIdx.x & 63;                                          \
  const int lane_in_group = threadIdx.x % GROUP;                              \
  const int group_in_wave = lane / GROUP;                                     \
  const int64_t col0 = col_off + (int64_t)lane_in_group * VEC;                \
  const bool active = !GUARD || (col0 < k);                                   \
                                                                              \
  const unsigned q0 = arrow_xcc_id() & 7;                                     \
  for (unsigned qi = 0; qi < 8; ++qi) {                                       \
    const unsigned q = (q0 + qi) & 7;                                         \
    const int64_t lo = qseg[q], hi = qseg[q + 1];                             \
    if (lo >= hi) continue;                                                   \
    for (;;) {                                                                \
      int grab = 0;                                                           \
      if (lane == 0) grab = atomicAdd(&qctr[q * 32], chunk_items);            \
      grab = __shfl(grab, 0, 64);                                             \
      const int64_t base = lo + grab;                                         \
      if (base >= hi) break;                                                  \
      const int64_t end = base + chunk_items < hi ? base + chunk_items : hi;  \
      spmm_process_items<T, VEC, GROUP, BETA, GUARD>(                         \
          base + group_in_wave, end, GROUPS_PER_WAVE, item_row, item_begin,   \
          item_end, X0, X1, C, k, col0, active, lane_in_group, nt_mode,       \
          EPILOGUE, a...);                                                    \
    }                                                                         \
  }

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_qw(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg,  // 9 segment bounds (items)
    int32_t *__restrict__ qctr,       // 8 counters, padded 32 ints apart
    int chunk_items,                  // per-WAVE grab size (items)
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode) {
  SPMM_QW_BODY(NoEpilogue{})
}

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_qw_affine(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg, int32_t *__restrict__ qctr,
    int chunk_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode,
    AffineEpilogue<T> ep) {
  SPMM_QW_BODY(ep)
}

template <typename T, int VEC, int GROUP, int BETA, bool GUARD, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void spmm_kernel_qw_affine_norm(
    const A *__restrict__... a,
    const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end,
    const int64_t *__restrict__ qseg, int32_t *__restrict__ qctr,
    int chunk_items,
    const T *__restrict__ X0, const T *__restrict__ X1,
    T *__restrict__ C, int64_t k, int64_t col_off, int nt_mode,
    AffineNormEpilogue<T> ep) {
  double sums[2] = {0.0, 0.0};
  SPMM_QW_BODY((AffineNormLane<T>{ep, sums}))
  norm_block_reduce(sums[0], sums[1], ep.acc);
}

template <typename T>
__global__ void zero_rows_kernel(T *__restrict__ C,
                                 const int32_t *__restrict__ rows,
                                 int64_t n_rows, int64_t k) {
  const int64_t total = n_rows * k;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k, j = t % k;
    C[(int64_t)rows[i] * k + j] = T(0);
  }
}

// bf16 split rows, after the SpMM launches of one call: round the fp32 sums
// in the scratch once, C[row] = bf16((BETA ? float(C[row]) : 0) + sum), and
// leave the scratch zero for the next call. k8 = k / 8; a thread moves one
// 16-byte piece of C and its 32 bytes of scratch.
template <int BETA>
__global__ void spmm_finalise_bf16(uint16_t *__restrict__ C,
                                   float *__restrict__ scratch,
                                   const int32_t *__restrict__ rows,
                                   int64_t n_rows, int64_t k8) {
  const int64_t total = n_rows * k8;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k8, j = t % k8;
    float4 *sp = reinterpret_cast<float4 *>(scratch) + 2 * t;
    const float4 s0 = sp[0], s1 = sp[1];
    float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint4 *cp = reinterpret_cast<uint4 *>(C) + (int64_t)rows[i] * k8 + j;
    if constexpr (BETA == 1) {
      const Float8 old = bf16x8_unpack(*cp);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = old[e] + s[e];
    }
    *cp = bf16x8_pack(s);
    sp[0] = sp[1] = float4{0.f, 0.f, 0.f, 0.f};
  }
}

// Affine step, fp32 / f64 split rows, before the SpMM launches of one call:
// the initialise pass that stands where zero_rows_kernel stands for the plain
// entry points. C[row] = gamma * R[row] at beta = 0 (zero when R is null),
// C[row] += gamma * R[row] at beta = 1; the items then add alpha * partial.
template <typename T>
__global__ void init_rows_affine_kernel(T *__restrict__ C,
                                        const T *__restrict__ R, T gamma,
                                        int beta,
                                        const int32_t *__restrict__ rows,
                                        int64_t n_rows, int64_t k) {
  const int64_t total = n_rows * k;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k, j = t % k;
    const int64_t at = (int64_t)rows[i] * k + j;
    const T v = R ? gamma * R[at] : T(0);
    C[at] = beta ? C[at] + v : v;
  }
}

// Affine step, bf16 split rows: spmm_finalise_bf16 with the epilogue,
// C[row] = bf16(alpha * sum + gamma * float(R[row]) + (BETA ? float(C[row])
// : 0)), one rounding per element; the scratch is left zero.
template <int BETA>
__global__ void spmm_finalise_affine_bf16(uint16_t *__restrict__ C,
                                          float *__restrict__ scratch,
                                          const int32_t *__restrict__ rows,
                                          int64_t n_rows, int64_t k8,
                                          const uint16_t *__restrict__ R,
                                          float alpha, float gamma) {
  const int64_t total = n_rows * k8;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k8, j = t % k8;
    float4 *sp = reinterpret_cast<float4 *>(scratch) + 2 * t;
    const float4 s0 = sp[0], s1 = sp[1];
    float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const int64_t at = (int64_t)rows[i] * k8 + j;
    uint4 *cp = reinterpret_cast<uint4 *>(C) + at;
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] *= alpha;
    if (R) {
      const Float8 r = bf16x8_unpack(reinterpret_cast<const uint4 *>(R)[at]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = fmaf(gamma, r[e], s[e]);
    }
    if constexpr (BETA == 1) {
      const Float8 old = bf16x8_unpack(*cp);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += old[e];
    }
    *cp = bf16x8_pack(s);
    sp[0] = sp[1] = float4{0.f, 0.f, 0.f, 0.f};
  }
}

// spmm_finalise_affine_bf16 at beta = 0 that also measures the split rows it
// finishes (the SpMM launches skipped them): the same arithmetic, written
// out again because the kernel above is to stay the instructions it was.
__global__ void spmm_finalise_affine_norm_bf16(
    uint16_t *__restrict__ C, float *__restrict__ scratch,
    const int32_t *__restrict__ rows, int64_t n_rows, int64_t k8,
    const uint16_t *__restrict__ R, float alpha, float gamma,
    const uint16_t *__restrict__ D, double *__restrict__ acc) {
  const int64_t total = n_rows * k8;
  double sums[2] = {0.0, 0.0};
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k8, j = t % k8;
    float4 *sp = reinterpret_cast<float4 *>(scratch) + 2 * t;
    const float4 s0 = sp[0], s1 = sp[1];
    float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const int64_t at = (int64_t)rows[i] * k8 + j;
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] *= alpha;
    if (R) {
      const Float8 r = bf16x8_unpack(reinterpret_cast<const uint4 *>(R)[at]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = fmaf(gamma, r[e], s[e]);
    }
    const uint4 packed = bf16x8_pack(s);
    const uint4 dv = D ? reinterpret_cast<const uint4 *>(D)[at] : uint4{};
    norm_add<float, 8>(sums, bf16x8_unpack(packed), bf16x8_unpack(dv));
    reinterpret_cast<uint4 *>(C)[at] = packed;
    sp[0] = sp[1] = float4{0.f, 0.f, 0.f, 0.f};
  }
  norm_block_reduce(sums[0], sums[1], acc);
}

// fp32 / f64 split rows of a measuring call, once after its last column-tile
// launch: the atomics have finished C[row], so read it back with D[row] over
// all k columns and add. Launched with BLOCK_THREADS threads.
template <typename T>
__global__ void diffnorm_split_rows_kernel(const T *__restrict__ C,
                                           const T *__restrict__ D,
                                           const int32_t *__restrict__ rows,
                                           int64_t n_rows, int64_t k,
                                           double *__restrict__ acc) {
  const int64_t total = n_rows * k;
  double sums[2] = {0.0, 0.0};
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k, j = t % k;
    const int64_t at = (int64_t)rows[i] * k + j;
    const T c = C[at], d = D ? D[at] : T(0);
    norm_add<T, 1>(sums, &c, &d);
  }
  norm_block_reduce(sums[0], sums[1], acc);
}

// The stand-alone form of the measure, over a contiguous n x k block: for
// results that no single launch finishes. Shaped like axpby_rows_kernel
// below (N elements = 16 bytes per thread when k allows, else one; D is null
// for d = 0), launched with BLOCK_THREADS threads.
template <typename T, int N>
__global__ void diffnorm_rows_kernel(const T *__restrict__ C,
                                     const T *__restrict__ D,
                                     int64_t total_vec,
                                     double *__restrict__ acc) {
  using P = Prec<T>;
  using Acc = typename P::Acc;
  double sums[2] = {0.0, 0.0};
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       t < total_vec; t += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (N == 1) {
      const T c = C[t], d = D ? D[t] : T(0);
      norm_add<Acc, 1>(sums, &c, &d);
    } else {
      using XV = typename P::template XV<N>;
      const XV cv = reinterpret_cast<const XV *>(C)[t];
      const XV dv = D ? reinterpret_cast<const XV *>(D)[t] : XV{};
      norm_add<Acc, N>(sums, P::template unpack<N>(cv),
                       P::template unpack<N>(dv));
    }
  }
  norm_block_reduce(sums[0], sums[1], acc);
}

constexpr int NORM_MAX_BLOCKS = 4096;  // 2 atomics per workgroup

template <typename T>
int launch_diffnorm(const char *who, const T *C, const T *D, int64_t n,
                    int64_t k, double *acc, hipStream_t stream) {
  if (n < 0 || k <= 0 || (n > 0 && !C)) {
    set_error(std::string(who) + ": bad arguments");
    return -1;
  }
  if (!acc) {
    set_error(std::string(who) + ": acc is NULL");
    return -7;
  }
  if (D && D == C) {
    set_error(std::string(who) + ": D must not be C");
    return -8;
  }
  if (n == 0) return 0;
  constexpr int N = 16 / sizeof(T);
  const bool vec = (k % N == 0);
  const int64_t total = vec ? n * (k / N) : n * k;
  int blocks = (int)std::min<int64_t>(
      (total + BLOCK_THREADS - 1) / BLOCK_THREADS, NORM_MAX_BLOCKS);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK_THREADS), 0, stream, C,
                       D, total, acc);
  };
  if constexpr (sizeof(T) == 2) {  // bf16: the caller checked k % 8 == 0
    launch(diffnorm_rows_kernel<T, N>);
  } else {
    if (vec) launch(diffnorm_rows_kernel<T, N>);
    else     launch(diffnorm_rows_kernel<T, 1>);
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

// The stand-alone tail of the affine step, C = alpha * C + gamma * R over a
// contiguous n x k block, for the engine layouts that do not fuse it into a
// launch. A thread moves N elements (16 bytes when k allows, else one); bf16
// computes in fp32 and rounds once. R is null when gamma == 0.
template <typename T, int N>
__global__ void axpby_rows_kernel(T *__restrict__ C, const T *__restrict__ R,
                                  int64_t total_vec,
                                  typename Prec<T>::Acc alpha,
                                  typename Prec<T>::Acc gamma) {
  using P = Prec<T>;
  using Acc = typename P::Acc;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       t < total_vec; t += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (N == 1) {
      Acc o = alpha * C[t];
      if (R) o = P::mad(gamma, R[t], o);
      C[t] = o;
    } else {
      using XV = typename P::template XV<N>;
      XV *cp = reinterpret_cast<XV *>(C) + t;
      const auto &c = P::template unpack<N>(*cp);
      Acc o[N];
#pragma unroll
      for (int j = 0; j < N; ++j) o[j] = alpha * c[j];
      if (R) {
        const XV rv = reinterpret_cast<const XV *>(R)[t];
        const auto &r = P::template unpack<N>(rv);
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = P::mad(gamma, r[j], o[j]);
      }
      *cp = P::template pack<N>(o);
    }
  }
}

template <typename T>
int launch_axpby(const char *who, T *C, const T *R, int64_t n, int64_t k,
                 double alpha, double gamma, hipStream_t stream) {
  using Acc = typename Prec<T>::Acc;
  if (n < 0 || k <= 0 || (n > 0 && !C)) {
    set_error(std::string(who) + ": bad arguments");
    return -1;
  }
  if (n == 0) return 0;
  if (!R && gamma != 0.0) {
    set_error(std::string(who) + ": R is NULL but gamma is not 0");
    return -4;
  }
  if (R && R == C) {
    set_error(std::string(who) + ": R must not be C");
    return -5;
  }
  constexpr int N = 16 / sizeof(T);
  const bool vec = (k % N == 0);
  const int64_t total = vec ? n * (k / N) : n * k;
  const int threads = 256;
  int blocks = (int)std::min<int64_t>((total + threads - 1) / threads, 16384);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, stream, C, R,
                       total, (Acc)alpha, (Acc)gamma);
  };
  if constexpr (sizeof(T) == 2) {  // bf16: the caller checked k % 8 == 0
    launch(axpby_rows_kernel<T, N>);
  } else {
    if (vec) launch(axpby_rows_kernel<T, N>);
    else     launch(axpby_rows_kernel<T, 1>);
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// Operator passes over the resident values (arrow_csr_sums, arrow_csr_scale):
// one streaming read (scale: and write) of the A stream, indexed exactly as
// the SpMM launches index C / R (output row of the item), X0 (col >= 0) and
// X1 (col < 0, at -col-1). One WAVE per work item, lanes strided over the
// item's nonzeros, so the fp32 pairs and the f64 cols / vals are read and
// written coalesced; waves stride over the items (the item index is
// wave-uniform, so every lane of a wave reaches every shuffle). Written once
// over the element type; A... is the mutable or const stream of Prec<T>.
// ---------------------------------------------------------------------------

constexpr int OPERATOR_MAX_BLOCKS = 4096;
constexpr int WAVES_PER_BLOCK = BLOCK_THREADS / 64;

// row_sum[out_row] += sum f(v), col_sum0[c] += f(v) (c >= 0),
// col_sum1[-c-1] += f(v) (c < 0); f = fabs when absolute. All in double. A
// null output is skipped. The row sum is reduced over the wave and added
// with one float64 atomic per item (a split row has several items); the
// column sums take one float64 hardware atomic per nonzero.
template <typename T, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void csr_sums_kernel(
    const int32_t *__restrict__ item_row,
    const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end, int64_t n_items, double *row_sum,
    double *col_sum0, double *col_sum1, int absolute,
    const A *__restrict__... a) {
  using P = Prec<T>;
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  for (int64_t it = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
       it < n_items; it += n_waves) {
    const int32_t row = item_row[it] & INT32_MAX;
    const int32_t b = item_begin[it], e = item_end[it];
    double s = 0.0;
    for (int32_t t = b + lane; t < e; t += 64) {
      const auto mine = P::load(0, t, a...);
      const int32_t c = P::own_col(mine);
      double v = (double)P::own_val(mine);
      if (absolute) v = fabs(v);
      s += v;
      if (c >= 0) {
        if (col_sum0) atomicAdd(col_sum0 + c, v);
      } else {
        if (col_sum1) atomicAdd(col_sum1 + -(c + 1), v);
      }
    }
    if (row_sum) {  // kernel-uniform
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0 && e > b) atomicAdd(row_sum + row, s);
    }
  }
}

// val = (T)(((double)val * r) * c): r = row_scale[out_row], loaded once per
// item, c = col_scale0[col] or col_scale1[-col-1]; a null vector is the
// factor 1. Two double multiplies in this order, one rounding to T.
template <typename T, typename... A>
__global__ __launch_bounds__(BLOCK_THREADS) void csr_scale_kernel(
    const int32_t *__restrict__ item_row,
    const int32_t *__restrict__ item_begin,
    const int32_t *__restrict__ item_end, int64_t n_items,
    const double *__restrict__ row_scale, const double *col_scale0,
    const double *col_scale1, A *__restrict__... a) {
  using P = Prec<T>;
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  for (int64_t it = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
       it < n_items; it += n_waves) {
    const int32_t b = item_begin[it], e = item_end[it];
    if (b >= e) continue;  // wave-uniform; no shuffle below
    const double r =
        row_scale ? row_scale[item_row[it] & INT32_MAX] : 1.0;
    for (int32_t t = b + lane; t < e; t += 64) {
      const auto mine = P::load(0, t, a...);
      const int32_t c = P::own_col(mine);
      double cf = 1.0;
      if (c >= 0) {
        if (col_scale0) cf = col_scale0[c];
      } else {
        if (col_scale1) cf = col_scale1[-(c + 1)];
      }
      const double v = ((double)P::own_val(mine) * r) * cf;
      P::store_val(t, c, (T)v, a...);
    }
  }
}

inline int operator_blocks(const CsrBlock &blk) {
  return (int)std::min<int64_t>(
      (blk.n_items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK,
      OPERATOR_MAX_BLOCKS);
}

template <typename T>
int launch_csr_sums(const CsrBlock &blk, double *row_sum, double *col_sum0,
                    double *col_sum1, int absolute, hipStream_t stream) {
  return Prec<T>::with_stream(blk, [&](auto *...a) {
    hipLaunchKernelGGL(
        (csr_sums_kernel<T, std::remove_pointer_t<decltype(a)>...>),
        dim3(operator_blocks(blk)), dim3(BLOCK_THREADS), 0, stream,
        (const int32_t *)blk.item_row, (const int32_t *)blk.item_begin,
        (const int32_t *)blk.item_end, blk.n_items, row_sum, col_sum0,
        col_sum1, absolute, a...);
    HIP_CHECK(hipGetLastError());
    return 0;
  });
}

template <typename T>
int launch_csr_scale(const CsrBlock &blk, const double *row_scale,
                     const double *col_scale0, const double *col_scale1,
                     hipStream_t stream) {
  return Prec<T>::with_stream(blk, [&](auto *...a) {
    hipLaunchKernelGGL(
        (csr_scale_kernel<T, std::remove_pointer_t<decltype(a)>...>),
        dim3(operator_blocks(blk)), dim3(BLOCK_THREADS), 0, stream,
        (const int32_t *)blk.item_row, (const int32_t *)blk.item_begin,
        (const int32_t *)blk.item_end, blk.n_items, row_scale, col_scale0,
        col_scale1, a...);
    HIP_CHECK(hipGetLastError());
    return 0;
  });
}

// ---------------------------------------------------------------------------
// Row gather / scatter / scatter-add (permutation routing on-device).
// ---------------------------------------------------------------------------

enum class RouteOp { Gather, Scatter, ScatterAdd };

// A lane moves N elements of T: 16 bytes when k allows, else one element.
// The float64 pure copies run the float kernels on rows of 2k floats, so
// only the adding forms are instantiated for double. bf16 rows (T =
// uint16_t raw bits, k % 8 == 0) likewise copy as k/2 floats; their adding
// forms take 8 bf16 of each side, add in fp32 and round once.
template <typename T, int N>
using RouteVec = std::conditional_t<
    N == 1, T,
    std::conditional_t<sizeof(T) == 2, uint4,
                       HIP_vector_type<std::conditional_t<sizeof(T) == 2, float, T>, N>>>;

template <typename T, int N>
__device__ __forceinline__ void route_add(RouteVec<T, N> *d,
                                          const RouteVec<T, N> &v) {
  if constexpr (sizeof(T) == 2) {
    static_assert(N == 8, "bf16 rows move 16 bytes per lane");
    const Float8 a = bf16x8_unpack(*d), b = bf16x8_unpack(v);
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = a[j] + b[j];
    *d = bf16x8_pack(sum);
  } else if constexpr (N == 1) {
    *d += v;
  } else {
    RouteVec<T, N> b = *d;
#pragma unroll
    for (int j = 0; j < N; ++j) b[j] += v[j];
    *d = b;
  }
}

template <typename T, int N, RouteOp OP>
__global__ void route_rows_kernel(T *__restrict__ dst,
                                  const T *__restrict__ src,
                                  const int64_t *__restrict__ idx, int64_t n,
                                  int64_t k_vec) {
  // k_vec = k / N; row r maps dst<->src[idx[r]]
  using VT = RouteVec<T, N>;
  const int64_t total = n * k_vec;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k_vec, j = t % k_vec;
    if constexpr (OP == RouteOp::Gather) {
      reinterpret_cast<VT *>(dst)[i * k_vec + j] =
          reinterpret_cast<const VT *>(src)[idx[i] * k_vec + j];
    } else if constexpr (OP == RouteOp::Scatter) {
      reinterpret_cast<VT *>(dst)[idx[i] * k_vec + j] =
          reinterpret_cast<const VT *>(src)[i * k_vec + j];
    } else {
      const VT v = reinterpret_cast<const VT *>(src)[i * k_vec + j];
      route_add<T, N>(reinterpret_cast<VT *>(dst) + idx[i] * k_vec + j, v);
    }
  }
}

// dst[dst_idx[i], :] (+)= src[src_idx[i], :] — fused gather+scatter for the
// rank-local share of the permutation exchange (one read + one write per
// element instead of a gather pass plus a scatter pass).
template <typename T, int N, bool ADD>
__global__ void permute_rows_kernel(T *__restrict__ dst,
                                    const T *__restrict__ src,
                                    const int64_t *__restrict__ dst_idx,
                                    const int64_t *__restrict__ src_idx,
                                    int64_t n, int64_t k_vec) {
  using VT = RouteVec<T, N>;
  const int64_t total = n * k_vec;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / k_vec, j = t % k_vec;
    const VT v = reinterpret_cast<const VT *>(src)[src_idx[i] * k_vec + j];
    VT *d = reinterpret_cast<VT *>(dst) + dst_idx[i] * k_vec + j;
    if constexpr (ADD) route_add<T, N>(d, v);
    else               *d = v;
  }
}

template <typename T, bool ADD>
int launch_permute(T *dst, const T *src, const int64_t *dst_idx,
                   const int64_t *src_idx, int64_t n, int64_t k,
                   hipStream_t stream) {
  if (n == 0) return 0;
  constexpr int N = 16 / sizeof(T);
  const bool vec = (k % N == 0);
  const int64_t k_vec = vec ? k / N : k;
  const int threads = 256;
  int blocks = (int)std::min<int64_t>((n * k_vec + threads - 1) / threads, 16384);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, stream, dst, src,
                       dst_idx, src_idx, n, k_vec);
  };
  if constexpr (sizeof(T) == 2) {  // bf16: the caller checked k % 8 == 0
    launch(permute_rows_kernel<T, N, ADD>);
  } else {
    if (vec) launch(permute_rows_kernel<T, N, ADD>);
    else     launch(permute_rows_kernel<T, 1, ADD>);
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T, RouteOp OP>
int launch_route(T *dst, const T *src, const int64_t *idx, int64_t n,
                 int64_t k, hipStream_t stream) {
  if (n == 0) return 0;
  constexpr int N = 16 / sizeof(T);
  const bool vec = (k % N == 0);
  const int64_t k_vec = vec ? k / N : k;
  const int64_t total = n * k_vec;
  const int threads = 256;
  int blocks = (int)std::min<int64_t>((total + threads - 1) / threads, 16384);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, stream, dst, src,
                       idx, n, k_vec);
  };
  if constexpr (sizeof(T) == 2) {  // bf16: the caller checked k % 8 == 0
    launch(route_rows_kernel<T, N, OP>);
  } else {
    if (vec) launch(route_rows_kernel<T, N, OP>);
    else     launch(route_rows_kernel<T, 1, OP>);
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// SpMM dispatch over (VEC, GROUP, BETA, GUARD)
// ---------------------------------------------------------------------------

// Kernel-tuning environment, read ONCE per process on first use (first
// arrow_spmm / arrow_spmm_dual / arrow_spmm_plan call). Changing a variable
// afterwards has no effect.
struct SpmmEnv {
  int g64;        // ARROW_SPMM_G64=1: k=128 as float2 x 64 lanes (A/B)
  int k16g8;      // ARROW_K16_G8=1: k=16 as float2 x 8 lanes (A/B, block-grab
                  // queue eligible)
  // Non-temporal pairs load + C store: default ON (+1.4-1.7 % at cfg4
  // with the queue scheduler — the once-read A stream and once-written C
  // stop evicting the X window; profiles/r01_nt_chunk_k32_ab.txt,
  // r01_colsort_nt_ab.txt). ARROW_SPMM_NT=0 restores cached accesses.
  int nt_mode;
  // ARROW_QUEUE: -1 unset (per-launch policy below), 0 forces grid-stride,
  // 1 forces queues.
  int queue_default;
  // Per-wave queue grabs (spmm_kernel_qw): no per-chunk block barrier.
  // Default AUTO (-1): wave variant at GROUP < 8 (k=16: measured +10% over
  // the fused grid-stride and +15% over the round-1 baseline,
  // profiles/r02_ab2_sweep.log k16_fused_q1_qw), block variant at
  // GROUP >= 8 (k=128: wave measured -17%, r02_ab1). ARROW_QWAVE=0/1
  // forces.
  int qwave;
  // policy default: queues need GROUP >= 4 AND enough work per structure —
  // below ~32M nnz (ARROW_Q_MIN_NNZ overrides) the per-grab overhead
  // outweighs the L2 window benefit (measured +54 % at k=128/cfg4, +18 %
  // at k=64, +2 % at k=32 same-box; profiles/r01_queue_chunk_sweep.txt,
  // r01_ksweep_queue_20M.txt)
  int64_t q_min_nnz;
  // Queue mode: size the grid to residency (8 blocks/CU fit at this
  // occupancy — 4 waves/WG, 8 waves/SIMD), not to the item count; chunk =
  // 4 rounds per grab (measured best on the fused cfg4 structure: 1/2/4 →
  // 4306/4450/4552 GF/s, profiles/r02_ab2_sweep.log).
  int q_chunk_mult;  // ARROW_Q_CHUNK
  int q_blocks;      // ARROW_Q_BLOCKS
  // per-wave grabs pull GROUPS_PER_WAVE-item rounds. Default 2 rounds —
  // the wave variant regresses at larger grabs (k=16: 1811 GF/s at 2 vs
  // 1342 at 4, 786 at 8 — its locality window is per-wave, so bigger
  // chunks smear it). ARROW_QW_CHUNK overrides.
  int qw_chunk_mult;
};

const SpmmEnv &spmm_env() {
  static const SpmmEnv env = [] {
    SpmmEnv v;
    const char *e = getenv("ARROW_SPMM_G64");
    v.g64 = (e && e[0] == '1') ? 1 : 0;
    e = getenv("ARROW_K16_G8");
    v.k16g8 = (e && e[0] == '1') ? 1 : 0;
    e = getenv("ARROW_SPMM_NT");
    v.nt_mode = (e && e[0] == '0') ? 0 : 1;
    e = getenv("ARROW_QUEUE");
    v.queue_default = (!e || !e[0]) ? -1 : (e[0] == '0') ? 0 : 1;
    e = getenv("ARROW_QWAVE");
    v.qwave = (!e || !e[0]) ? -1 : (e[0] == '1') ? 1 : 0;
    e = getenv("ARROW_Q_MIN_NNZ");
    v.q_min_nnz = e ? (int64_t)atoll(e) : (32LL << 20);
    e = getenv("ARROW_Q_CHUNK");
    v.q_chunk_mult = e ? std::max(1, atoi(e)) : 4;
    e = getenv("ARROW_Q_BLOCKS");
    v.q_blocks = e ? std::max(8, atoi(e)) : 2048;
    e = getenv("ARROW_QW_CHUNK");
    v.qw_chunk_mult = e ? std::max(1, atoi(e)) : 2;
    return v;
  }();
  return env;
}

enum Scheduler { SCHED_GRID_STRIDE = 0, SCHED_QUEUE_BLOCK = 1, SCHED_QUEUE_WAVE = 2 };
constexpr int GRID_STRIDE_MAX_BLOCKS = 8192;

// The whole launch decision for one arrow_spmm call. launch_spmm_vg consumes
// it; arrow_spmm_plan exports it.
struct SpmmPlan {
  int vec;
  int group;
  int scheduler;    // Scheduler
  int nt_mode;
  int chunk_items;  // items per queue grab as launched (0 for grid-stride)
  int grid_cap;     // max workgroups for the chosen scheduler
  int n_launches;   // col_off launches = ceil(k / (group * vec))
};

// A lane holds VEC elements, 16 bytes when k allows: float4 / double2, and
// always 8 bf16 (dtype 16: the callers refuse k % 8 != 0).
// ARROW_SPMM_G64 / ARROW_K16_G8 are fp32 layout experiments and do not
// apply to float64 or to bf16 features.
void pick_cfg(int64_t k, int dtype, int *vec_out, int *group_out) {
  const SpmmEnv &env = spmm_env();
  int vec;
  if (dtype == 16) {
    vec = 8;
  } else if (dtype == 64) {
    vec = (k % 2 == 0) ? 2 : 1;
  } else {
    if (env.g64 && k == 128) { *vec_out = 2; *group_out = 64; return; }
    if (env.k16g8 && k == 16) { *vec_out = 2; *group_out = 8; return; }
    vec = (k % 4 == 0) ? 4 : (k % 2 == 0) ? 2 : 1;
  }
  const int64_t lanes_needed = (k + vec - 1) / vec;
  int group = 1;
  while (group < lanes_needed && group < 64) group <<= 1;
  *vec_out = vec;
  *group_out = group;
}

// queue_mode: the structure's arrow_csr_set_queue mode (-1 follows
// ARROW_QUEUE); q_blocks_override: its arrow_csr_set_qblocks value (0 = none).
// dtype 32, 64 or 16 (bf16 features) only selects the (vec, group) layout:
// the scheduler policy and its thresholds are shared (a lane is 16 bytes in
// every precision, so GROUP-based thresholds carry over by row bytes;
// measured for fp32 only).
SpmmPlan spmm_plan(int64_t k, int64_t nnz, int queue_mode,
                   int q_blocks_override, int dtype = 32) {
  const SpmmEnv &env = spmm_env();
  SpmmPlan p;
  pick_cfg(k, dtype, &p.vec, &p.group);
  p.nt_mode = env.nt_mode;
  const int qd = queue_mode >= 0 ? (queue_mode ? 1 : 0) : env.queue_default;
  const bool useq = qd >= 0 ? (qd == 1)
                            : (p.group >= 4 && nnz >= env.q_min_nnz);
  const bool qwave = env.qwave >= 0 ? (env.qwave == 1) : (p.group < 8);
  if (!useq) {
    p.scheduler = SCHED_GRID_STRIDE;
    p.chunk_items = 0;
    p.grid_cap = GRID_STRIDE_MAX_BLOCKS;
  } else {
    p.scheduler = qwave ? SCHED_QUEUE_WAVE : SCHED_QUEUE_BLOCK;
    p.chunk_items = qwave ? (64 / p.group) * env.qw_chunk_mult
                          : (BLOCK_THREADS / p.group) * env.q_chunk_mult;
    p.grid_cap = q_blocks_override > 0 ? q_blocks_override : env.q_blocks;
  }
  const int64_t span = (int64_t)p.group * p.vec;
  p.n_launches = (int)((k + span - 1) / span);
  return p;
}

// a...: the structure's A-stream device pointers (Prec<T>::with_stream)
// The entry symbol of a scheduler for the epilogue EP: the plain kernel, its
// _affine form or its _affine_norm form.
template <typename EP, typename T, int VEC, int GROUP, int BETA, bool GUARD,
          typename... A>
constexpr auto grid_kernel() {
  if constexpr (std::is_same_v<EP, NoEpilogue>)
    return &spmm_kernel<T, VEC, GROUP, BETA, GUARD, A...>;
  else if constexpr (std::is_same_v<EP, AffineEpilogue<T>>)
    return &spmm_kernel_affine<T, VEC, GROUP, BETA, GUARD, A...>;
  else
    return &spmm_kernel_affine_norm<T, VEC, GROUP, BETA, GUARD, A...>;
}
template <typename EP, typename T, int VEC, int GROUP, int BETA, bool GUARD,
          typename... A>
constexpr auto q_kernel() {
  if constexpr (std::is_same_v<EP, NoEpilogue>)
    return &spmm_kernel_q<T, VEC, GROUP, BETA, GUARD, A...>;
  else if constexpr (std::is_same_v<EP, AffineEpilogue<T>>)
    return &spmm_kernel_q_affine<T, VEC, GROUP, BETA, GUARD, A...>;
  else
    return &spmm_kernel_q_affine_norm<T, VEC, GROUP, BETA, GUARD, A...>;
}
template <typename EP, typename T, int VEC, int GROUP, int BETA, bool GUARD,
          typename... A>
constexpr auto qw_kernel() {
  if constexpr (std::is_same_v<EP, NoEpilogue>)
    return &spmm_kernel_qw<T, VEC, GROUP, BETA, GUARD, A...>;
  else if constexpr (std::is_same_v<EP, AffineEpilogue<T>>)
    return &spmm_kernel_qw_affine<T, VEC, GROUP, BETA, GUARD, A...>;
  else
    return &spmm_kernel_qw_affine_norm<T, VEC, GROUP, BETA, GUARD, A...>;
}

// ep: NoEpilogue{} for the plain entry points, else the affine step's
template <typename T, int VEC, int GROUP, typename EP, typename... A>
int launch_spmm_vg(const CsrBlock &blk, const SpmmPlan &plan, const T *X0,
                   const T *X1, T *C, int64_t k, int beta, hipStream_t stream,
                   const EP &ep, const A *... a) {
  constexpr bool AFFINE = !std::is_same_v<EP, NoEpilogue>;
  constexpr bool NORM = std::is_same_v<EP, AffineNormEpilogue<T>>;
  constexpr int GROUPS_PER_BLOCK = BLOCK_THREADS / GROUP;
  const int nt_mode = plan.nt_mode;
  const bool useq = plan.scheduler != SCHED_GRID_STRIDE;
  const bool qwave = plan.scheduler == SCHED_QUEUE_WAVE;
  if (useq && !(blk.qseg && blk.qctr)) {
    set_error(std::string("arrow_spmm") + Prec<T>::suffix +
              ": structure has no queue segments");
    return -1;
  }
  int blocks = (int)std::min<int64_t>(
      (blk.n_items + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK, plan.grid_cap);
  if (blocks < 1) blocks = 1;
  const int64_t span = (int64_t)GROUP * VEC;
  for (int64_t col_off = 0; col_off < k; col_off += span) {
    const bool guard = (col_off + span > k);
    auto run = [&](auto kern) {
      if constexpr (AFFINE) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK_THREADS), 0, stream,
                           a..., blk.item_row, blk.item_begin,
                           blk.item_end, blk.n_items, X0, X1, C, k, col_off,
                           blk.xcd_remap, nt_mode, ep);
      } else {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK_THREADS), 0, stream,
                           a..., blk.item_row, blk.item_begin,
                           blk.item_end, blk.n_items, X0, X1, C, k, col_off,
                           blk.xcd_remap, nt_mode);
      }
    };
    auto runq = [&](auto kern, int chunk) {
      if constexpr (AFFINE) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK_THREADS), 0, stream,
                           a..., blk.item_row, blk.item_begin,
                           blk.item_end, blk.qseg, blk.qctr, chunk,
                           X0, X1, C, k, col_off, nt_mode, ep);
      } else {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK_THREADS), 0, stream,
                           a..., blk.item_row, blk.item_begin,
                           blk.item_end, blk.qseg, blk.qctr, chunk,
                           X0, X1, C, k, col_off, nt_mode);
      }
    };
    // the launch for a compile-time beta; the measuring kernels exist at
    // beta = 0 only (their entry points refuse any other)
    auto go = [&](auto beta_c) {
      constexpr int BETA = decltype(beta_c)::value;
      if (useq && qwave) {
        if (guard) runq(qw_kernel<EP, T, VEC, GROUP, BETA, true, A...>(), plan.chunk_items);
        else       runq(qw_kernel<EP, T, VEC, GROUP, BETA, false, A...>(), plan.chunk_items);
      } else if (useq) {
        if (guard) runq(q_kernel<EP, T, VEC, GROUP, BETA, true, A...>(), plan.chunk_items);
        else       runq(q_kernel<EP, T, VEC, GROUP, BETA, false, A...>(), plan.chunk_items);
      } else {
        if (guard) run(grid_kernel<EP, T, VEC, GROUP, BETA, true, A...>());
        else       run(grid_kernel<EP, T, VEC, GROUP, BETA, false, A...>());
      }
    };
    if (useq)
      HIP_CHECK(hipMemsetAsync(blk.qctr, 0, 8 * 32 * sizeof(int32_t), stream));
    if constexpr (NORM) {
      go(std::integral_constant<int, 0>{});
    } else {
      if (beta == 0) go(std::integral_constant<int, 0>{});
      else           go(std::integral_constant<int, 1>{});
    }
    HIP_CHECK(hipGetLastError());
  }
  return 0;
}

template <typename T, int VEC, typename EP, typename... A>
int launch_spmm_v(const CsrBlock &blk, const SpmmPlan &plan, const T *X0,
                  const T *X1, T *C, int64_t k, int beta, hipStream_t stream,
                  const EP &ep, const A *... a) {
  switch (plan.group) {
    case 1:  return launch_spmm_vg<T, VEC, 1>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    case 2:  return launch_spmm_vg<T, VEC, 2>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    case 4:  return launch_spmm_vg<T, VEC, 4>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    case 8:  return launch_spmm_vg<T, VEC, 8>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    case 16: return launch_spmm_vg<T, VEC, 16>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    case 32: return launch_spmm_vg<T, VEC, 32>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
    default: return launch_spmm_vg<T, VEC, 64>(blk, plan, X0, X1, C, k, beta, stream, ep, a...);
  }
}

// arrow_spmm_dual / arrow_spmm_dual_f64. Error texts name the entry point
// family of T ("arrow_spmm" + suffix) and, for a handle of the other
// precision, the family it belongs to.
// bf16 features need k % 8 == 0: a row is then a whole number of 16-byte
// lanes and 16-byte aligned. The text names the rule.
bool bf16_k_ok(const std::string &who, int64_t k) {
  if (k % 8 == 0) return true;
  set_error(who + ": bfloat16 features need k % 8 == 0 (a lane moves 8 bf16 "
            "= 16 bytes, rows must be 16-byte aligned); got k = " +
            std::to_string(k));
  return false;
}

// The structure's fp32 scratch for bf16 split rows, n_split_rows x k floats,
// zero between launches: allocated on first need, grown when a wider k
// comes, never shrunk. hipMalloc is not legal under stream capture, so the
// first launch at a given k must come before any capture.
int ensure_bf16_scratch(CsrBlock &blk, int64_t k, hipStream_t stream) {
  if (blk.n_split_rows == 0 || blk.scratch_k >= k) return 0;
  float *p = nullptr;
  const size_t bytes = (size_t)blk.n_split_rows * (size_t)k * sizeof(float);
  HIP_CHECK(hipMalloc((void **)&p, bytes));
  if (blk.bf16_scratch) {
    // launches that use the old one may still be in flight
    HIP_CHECK(hipStreamSynchronize(stream));
    (void)hipFree(blk.bf16_scratch);
  }
  blk.bf16_scratch = p;
  blk.scratch_k = k;
  HIP_CHECK(hipMemsetAsync(p, 0, bytes, stream));
  return 0;
}

// ep: NoEpilogue{} (arrow_spmm*), or the affine step's R, alpha and gamma
// (arrow_spmm*_affine*; `gamma_given` is the caller's gamma before the cast
// to the accumulator type, for the R == NULL rule).
template <typename T, typename EP = NoEpilogue>
int spmm_dual_impl(int64_t handle, const T *X0_dev, const T *X1_dev, T *C_dev,
                   int64_t k, int beta, void *stream_v, const EP &ep = EP{},
                   double gamma_given = 0.0) {
  using P = Prec<T>;
  using Other = Prec<std::conditional_t<P::dtype == 32, double, float>>;
  constexpr bool BF16 = std::is_same_v<T, uint16_t>;
  constexpr bool AFFINE = !std::is_same_v<EP, NoEpilogue>;
  constexpr bool NORM = std::is_same_v<EP, AffineNormEpilogue<T>>;
  constexpr int plan_dtype = BF16 ? 16 : P::dtype;
  const std::string who =
      std::string(NORM ? "arrow_spmm_affine_norm"
                       : AFFINE ? "arrow_spmm_affine" : "arrow_spmm") +
      P::suffix;
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error(who + ": bad handle");
    return -1;
  }
  if (k <= 0 || !X0_dev || !X1_dev || !C_dev) {
    set_error(who + ": bad arguments");
    return -1;
  }
  CsrBlock &blk = it->second;
  if (blk.dtype != P::dtype) {
    const std::string o = Other::suffix;
    set_error(who + ": handle holds a float" + std::to_string(Other::dtype) +
              " structure (arrow_csr_create" + o + ") but was passed to the " +
              P::name + " entry point" +
              (BF16 ? ", which takes a float32 structure (arrow_csr_create*)"
                    : "") +
              "; use arrow_spmm" + o + " / arrow_spmm_dual" + o);
    return -2;
  }
  hipStream_t stream = (hipStream_t)stream_v;
  if constexpr (BF16) {
    if (!bf16_k_ok(who, k)) return -3;
  }
  if constexpr (AFFINE) {
    if (!ep.R && gamma_given != 0.0) {
      set_error(who + ": R is NULL but gamma is not 0");
      return -4;
    }
    if (ep.R && ep.R == C_dev) {
      set_error(who + ": R must not be C (X may alias R)");
      return -5;
    }
    if (NORM ? beta != 0 : (beta != 0 && beta != 1)) {
      set_error(who + ": beta must be 0" + (NORM ? "" : " or 1") + ", got " +
                std::to_string(beta));
      return -6;
    }
  }
  if constexpr (NORM) {
    if (!ep.acc) {
      set_error(who + ": acc is NULL");
      return -7;
    }
    if (ep.D && ep.D == C_dev) {
      set_error(who + ": D must not be C (D may alias X or R)");
      return -8;
    }
  }
  if constexpr (BF16) {
    if (ensure_bf16_scratch(blk, k, stream)) return -1;
  }

  // beta=0: split rows are accumulated with atomics, so pre-zero them (bf16
  // split rows go through the scratch and are written whole at the end).
  // Affine: the same pass initialises them with gamma * R (+ C) instead.
  if constexpr (AFFINE && !BF16) {
    if (blk.n_split_rows > 0 && (beta == 0 || ep.R)) {
      const int64_t total = blk.n_split_rows * k;
      int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
      hipLaunchKernelGGL(init_rows_affine_kernel<T>, dim3(blocks), dim3(256),
                         0, stream, C_dev, ep.R, ep.gamma, beta,
                         blk.split_rows, blk.n_split_rows, k);
      HIP_CHECK(hipGetLastError());
    }
  } else if constexpr (!BF16) {
    if (beta == 0 && blk.n_split_rows > 0) {
      const int64_t total = blk.n_split_rows * k;
      int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
      hipLaunchKernelGGL(zero_rows_kernel<T>, dim3(blocks), dim3(256), 0,
                         stream, C_dev, blk.split_rows, blk.n_split_rows, k);
      HIP_CHECK(hipGetLastError());
    }
  }

  const SpmmPlan plan =
      spmm_plan(k, blk.nnz, blk.queue_mode, blk.q_blocks, plan_dtype);
  const int rc = P::with_stream(blk, [&](const auto *... a) {
    if constexpr (BF16) {
      return launch_spmm_v<T, 8>(blk, plan, X0_dev, X1_dev, C_dev, k, beta, stream, ep, a...);
    } else {
      if constexpr (P::dtype == 32) {
        if (plan.vec == 4)
          return launch_spmm_v<T, 4>(blk, plan, X0_dev, X1_dev, C_dev, k, beta, stream, ep, a...);
      }
      if (plan.vec == 2)
        return launch_spmm_v<T, 2>(blk, plan, X0_dev, X1_dev, C_dev, k, beta, stream, ep, a...);
      return launch_spmm_v<T, 1>(blk, plan, X0_dev, X1_dev, C_dev, k, beta, stream, ep, a...);
    }
  });
  if constexpr (BF16) {
    if (rc == 0 && blk.n_split_rows > 0) {
      const int64_t total = blk.n_split_rows * (k / 8);
      int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
      auto fin = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, stream, C_dev,
                           blk.bf16_scratch, blk.split_rows, blk.n_split_rows,
                           k / 8);
      };
      auto fin_affine = [&](auto kern) {
        if constexpr (AFFINE) {
          hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, stream, C_dev,
                             blk.bf16_scratch, blk.split_rows,
                             blk.n_split_rows, k / 8, ep.R, ep.alpha,
                             ep.gamma);
        }
      };
      if constexpr (NORM) {
        hipLaunchKernelGGL(spmm_finalise_affine_norm_bf16, dim3(blocks),
                           dim3(BLOCK_THREADS), 0, stream, C_dev,
                           blk.bf16_scratch, blk.split_rows, blk.n_split_rows,
                           k / 8, ep.R, ep.alpha, ep.gamma, ep.D, ep.acc);
      } else if constexpr (AFFINE) {
        if (beta == 0) fin_affine(spmm_finalise_affine_bf16<0>);
        else           fin_affine(spmm_finalise_affine_bf16<1>);
      } else {
        if (beta == 0) fin(spmm_finalise_bf16<0>);
        else           fin(spmm_finalise_bf16<1>);
      }
      HIP_CHECK(hipGetLastError());
    }
  } else if constexpr (NORM) {
    // the split rows the launches skipped, now that their atomics are in
    if (rc == 0 && blk.n_split_rows > 0) {
      const int64_t total = blk.n_split_rows * k;
      int blocks = (int)std::min<int64_t>(
          (total + BLOCK_THREADS - 1) / BLOCK_THREADS, NORM_MAX_BLOCKS);
      hipLaunchKernelGGL(diffnorm_split_rows_kernel<T>, dim3(blocks),
                         dim3(BLOCK_THREADS), 0, stream, (const T *)C_dev,
                         ep.D, blk.split_rows, blk.n_split_rows, k, ep.acc);
      HIP_CHECK(hipGetLastError());
    }
  }
  return rc;
}

int spmm_plan_export(const char *who, int dtype, int64_t k, int64_t nnz,
                     int queue_mode, int32_t *out, int n_out) {
  if (k <= 0 || nnz < 0 || !out || n_out < 0) {
    set_error(std::string(who) + ": bad arguments");
    return -1;
  }
  if (dtype == 16 && !bf16_k_ok(who, k)) return -3;
  const SpmmPlan p = spmm_plan(k, nnz, queue_mode, 0, dtype);
  const int32_t fields[ARROW_PLAN_FIELDS] = {
      p.vec, p.group, p.scheduler, p.nt_mode, p.chunk_items, p.grid_cap,
      p.n_launches};
  for (int i = 0; i < n_out && i < ARROW_PLAN_FIELDS; ++i) out[i] = fields[i];
  return ARROW_PLAN_FIELDS;
}

// arrow_spmm*_affine*: the caller's double alpha and gamma, cast once to the
// accumulator type of T
template <typename T>
int spmm_affine(int64_t handle, const T *X0, const T *X1, T *C, const T *R,
                int64_t k, double alpha, double gamma, int beta,
                void *stream) {
  using Acc = typename Prec<T>::Acc;
  const AffineEpilogue<T> ep{R, (Acc)alpha, (Acc)gamma};
  return spmm_dual_impl<T>(handle, X0, X1, C, k, beta, stream, ep, gamma);
}

// arrow_spmm*_affine_norm*: the affine step plus D and the accumulator pair
template <typename T>
int spmm_affine_norm(int64_t handle, const T *X0, const T *X1, T *C,
                     const T *R, const T *D, double *acc, int64_t k,
                     double alpha, double gamma, int beta, void *stream) {
  using Acc = typename Prec<T>::Acc;
  const AffineNormEpilogue<T> ep{R, (Acc)alpha, (Acc)gamma, D, acc};
  return spmm_dual_impl<T>(handle, X0, X1, C, k, beta, stream, ep, gamma);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int arrow_abi_version(void) { return ARROW_ABI_VERSION; }

const char *arrow_last_error(void) { return g_last_error.c_str(); }

int arrow_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int arrow_set_device(int device) {
  HIP_CHECK(hipSetDevice(device));
  return 0;
}

int arrow_synchronize(void) {
  HIP_CHECK(hipDeviceSynchronize());
  return 0;
}

static int64_t csr_create_impl(int64_t rows, int64_t cols, int64_t nnz,
                               const int64_t *indptr, const int32_t *indices,
                               const void *data, const int64_t *row_ids,
                               int flags = 0, int dtype = 32) {
  if (rows < 0 || cols < 0 || nnz < 0 || (rows > 0 && !indptr)) {
    set_error("arrow_csr_create: bad arguments");
    return -1;
  }
  if (nnz > INT32_MAX) {
    set_error("arrow_csr_create: nnz exceeds int32 (per-block limit)");
    return -1;
  }
  // rows, columns and output row ids travel as int32 (the work items keep
  // bit 31 of the row for the split flag): refuse what does not fit, before
  // anything is allocated
  if (rows > INT32_MAX || cols > INT32_MAX) {
    set_error("arrow_csr_create: " +
              std::string(rows > INT32_MAX ? "rows " : "cols ") +
              std::to_string(rows > INT32_MAX ? rows : cols) +
              " exceeds int32 (per-block limit)");
    return -1;
  }
  if (row_ids) {
    for (int64_t r = 0; r < rows; ++r) {
      if (row_ids[r] < 0 || row_ids[r] > INT32_MAX) {
        set_error("arrow_csr_create: row id " + std::to_string(row_ids[r]) +
                  " at row " + std::to_string(r) +
                  (row_ids[r] < 0 ? " is negative (output row ids are int32)"
                                  : " exceeds int32"));
        return -1;
      }
    }
  }
  CsrBlock blk;
  blk.rows = rows;
  blk.cols = cols;
  blk.nnz = nnz;
  blk.dtype = dtype;

  // Build work items on the host: every row gets at least one item; rows
  // with > SEG_NNZ nonzeros are split and marked atomic (bit 31).
  std::vector<int32_t> item_row, item_begin, item_end, split_rows;
  item_row.reserve(rows + nnz / SEG_NNZ + 1);
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t b = indptr[r], e = indptr[r + 1];
    // row_ids (optional) maps structure-row -> output C row, enabling
    // reordered layouts (e.g. the hub-sorted X_0 structure)
    const int32_t out_row = (int32_t)(row_ids ? row_ids[r] : r);
    if (e - b <= SEG_NNZ) {
      item_row.push_back(out_row);
      item_begin.push_back((int32_t)b);
      item_end.push_back((int32_t)e);
    } else {
      split_rows.push_back(out_row);
      for (int64_t s = b; s < e; s += SEG_NNZ) {
        item_row.push_back(out_row | INT32_MIN);
        item_begin.push_back((int32_t)s);
        item_end.push_back((int32_t)std::min<int64_t>(s + SEG_NNZ, e));
      }
    }
  }
  blk.n_items = (int64_t)item_row.size();
  blk.n_split_rows = (int64_t)split_rows.size();
  // the device table: the count, then the rows ascending (their order does
  // not matter to the pre-zero pass; the bf16 kernels search them)
  std::sort(split_rows.begin(), split_rows.end());
  split_rows.insert(split_rows.begin(), (int32_t)blk.n_split_rows);

  // ARROW_CSR_COL_ITEMS: order work items by their first column instead of
  // by row. For hub-heavy structures (the first block-row: long CSR rows
  // split into column-contiguous items) this makes a queue segment a
  // COLUMN window of X, so the ~concurrent hub-row streams share the
  // XCD's L2. Output correctness is order-independent (each non-split row
  // appears once; split rows accumulate atomically either way).
  // Stable-sort the items [lo, hi) by their first column (empty items last).
  auto sort_items_by_first_col = [&](int64_t lo, int64_t hi) {
    auto first_col = [&](int64_t i) {
      return item_begin[(size_t)i] < item_end[(size_t)i]
                 ? indices[item_begin[(size_t)i]]
                 : INT32_MAX;
    };
    std::vector<int64_t> order((size_t)(hi - lo));
    for (int64_t i = lo; i < hi; ++i) order[(size_t)(i - lo)] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      return first_col(a) < first_col(b);
    });
    std::vector<int32_t> r2(order.size()), b2(order.size()), e2(order.size());
    for (size_t i = 0; i < order.size(); ++i) {
      r2[i] = item_row[(size_t)order[i]];
      b2[i] = item_begin[(size_t)order[i]];
      e2[i] = item_end[(size_t)order[i]];
    }
    std::copy(r2.begin(), r2.end(), item_row.begin() + (size_t)lo);
    std::copy(b2.begin(), b2.end(), item_begin.begin() + (size_t)lo);
    std::copy(e2.begin(), e2.end(), item_end.begin() + (size_t)lo);
  };
  if (flags & 1) sort_items_by_first_col(0, blk.n_items);

  // nnz-balanced contiguous item segments for the per-XCD queue scheduler
  // (items are in row order — or column order with flags&1 — so a segment
  // is a contiguous window of X)
  int64_t qseg_h[9];
  {
    // weight = nnz + 1 per item: balances by data volume while keeping
    // empty/short rows (fixed per-item overhead) spread across queues
    const int64_t n_it = blk.n_items;
    const int64_t total_w = nnz + n_it;
    int64_t cum = 0, target_q = 1;
    qseg_h[0] = 0;
    for (int64_t i = 0; i < n_it && target_q < 8; ++i) {
      cum += (item_end[(size_t)i] - item_begin[(size_t)i]) + 1;
      while (target_q < 8 && cum * 8 >= total_w * target_q) {
        qseg_h[target_q++] = i + 1;
      }
    }
    while (target_q <= 8) qseg_h[target_q++] = n_it;
  }

  // flags&2: TWO-LEVEL hub ordering — keep the 8 nnz-balanced ROW segments
  // (so each XCD still owns a contiguous C range and load stays balanced),
  // then sort the items WITHIN each segment by first column: an XCD's
  // queue walk becomes a column-window sweep of X while its C writes stay
  // inside the segment's row range. Order-independent for correctness
  // (each non-split row appears once; split rows accumulate atomically).
  if (flags & 2) {
    for (int q = 0; q < 8; ++q) sort_items_by_first_col(qseg_h[q], qseg_h[q + 1]);
  }

  // fp32: pack (col, val) into 8-byte pairs for the staged kernel loads.
  // float64: the caller's arrays are the resident layout as they are
  // (split int32 cols[] + double vals[])
  std::vector<int2> pairs(dtype == 32 ? (size_t)nnz : 0);
  if (dtype == 32) {
    const float *data32 = static_cast<const float *>(data);
    for (int64_t t = 0; t < nnz; ++t) {
      pairs[(size_t)t].x = indices[t];
      float v = data32[t];
      pairs[(size_t)t].y = *reinterpret_cast<const int32_t *>(&v);
    }
  }

  auto upload = [&](void **dst, const void *src, size_t bytes) -> int {
    if (bytes == 0) { *dst = nullptr; return 0; }
    HIP_CHECK(hipMalloc(dst, bytes));
    HIP_CHECK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  if (upload((void **)&blk.pairs, pairs.data(), pairs.size() * sizeof(int2)) ||
      (dtype == 64 &&
       (upload((void **)&blk.cols64, indices, (size_t)nnz * sizeof(int32_t)) ||
        upload((void **)&blk.vals64, data, (size_t)nnz * sizeof(double)))) ||
      upload((void **)&blk.item_row, item_row.data(), item_row.size() * 4) ||
      upload((void **)&blk.item_begin, item_begin.data(), item_begin.size() * 4) ||
      upload((void **)&blk.item_end, item_end.data(), item_end.size() * 4) ||
      upload((void **)&blk.split_tab, split_rows.data(), split_rows.size() * 4) ||
      upload((void **)&blk.qseg, qseg_h, sizeof(qseg_h))) {
    return -1;
  }
  blk.split_rows = blk.split_tab + 1;
  HIP_CHECK(hipMalloc((void **)&blk.qctr, 8 * 32 * sizeof(int32_t)));
  const int64_t h = g_next_handle++;
  g_blocks.emplace(h, blk);
  return h;
}

int64_t arrow_csr_create(int64_t rows, int64_t cols, int64_t nnz,
                         const int64_t *indptr, const int32_t *indices,
                         const float *data) {
  return csr_create_impl(rows, cols, nnz, indptr, indices, data, nullptr);
}

int64_t arrow_csr_create_rows(int64_t rows, int64_t cols, int64_t nnz,
                              const int64_t *indptr, const int32_t *indices,
                              const float *data, const int64_t *row_ids) {
  return csr_create_impl(rows, cols, nnz, indptr, indices, data, row_ids);
}

int64_t arrow_csr_create_opts(int64_t rows, int64_t cols, int64_t nnz,
                              const int64_t *indptr, const int32_t *indices,
                              const float *data, const int64_t *row_ids,
                              int flags) {
  return csr_create_impl(rows, cols, nnz, indptr, indices, data, row_ids,
                         flags);
}

int arrow_csr_destroy(int64_t handle) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_destroy: bad handle");
    return -1;
  }
  CsrBlock &b = it->second;
  for (void *p : {(void *)b.pairs, (void *)b.cols64, (void *)b.vals64,
                  (void *)b.item_row,
                  (void *)b.item_begin, (void *)b.item_end,
                  (void *)b.split_tab, (void *)b.bf16_scratch,
                  (void *)b.qseg, (void *)b.qctr}) {
    if (p) (void)hipFree(p);
  }
  g_blocks.erase(it);
  return 0;
}

int64_t arrow_csr_create_f64(int64_t rows, int64_t cols, int64_t nnz,
                             const int64_t *indptr, const int32_t *indices,
                             const double *data, const int64_t *row_ids,
                             int flags) {
  return csr_create_impl(rows, cols, nnz, indptr, indices, data, row_ids,
                         flags, 64);
}

int arrow_csr_dtype(int64_t handle) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_dtype: bad handle");
    return -1;
  }
  return it->second.dtype;
}

int64_t arrow_csr_nnz(int64_t handle) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) return -1;
  return it->second.nnz;
}

int arrow_csr_set_xcd_remap(int64_t handle, int enable) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_set_xcd_remap: bad handle");
    return -1;
  }
  it->second.xcd_remap = enable ? 1 : 0;
  return 0;
}

int arrow_csr_set_queue(int64_t handle, int mode) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_set_queue: bad handle");
    return -1;
  }
  it->second.queue_mode = mode < 0 ? -1 : (mode ? 1 : 0);
  return 0;
}

int arrow_csr_set_qblocks(int64_t handle, int blocks) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_set_qblocks: bad handle");
    return -1;
  }
  it->second.q_blocks = blocks > 0 ? blocks : 0;
  return 0;
}

// ABI 1007: sums and in-place rescale of the resident values. Both dispatch
// on the handle's precision tag; neither allocates nor reads on the host.
int arrow_csr_sums(int64_t handle, double *row_sum_dev, double *col_sum0_dev,
                   double *col_sum1_dev, int absolute, void *stream_v) {
  if (!row_sum_dev && !col_sum0_dev && !col_sum1_dev) {
    set_error("arrow_csr_sums: row_sum, col_sum0 and col_sum1 are all NULL");
    return -7;
  }
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_sums: bad handle");
    return -1;
  }
  const CsrBlock &blk = it->second;
  if (blk.nnz == 0) return 0;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  return blk.dtype == 64
             ? launch_csr_sums<double>(blk, row_sum_dev, col_sum0_dev,
                                       col_sum1_dev, absolute, stream)
             : launch_csr_sums<float>(blk, row_sum_dev, col_sum0_dev,
                                      col_sum1_dev, absolute, stream);
}

int arrow_csr_scale(int64_t handle, const double *row_scale_dev,
                    const double *col_scale0_dev, const double *col_scale1_dev,
                    void *stream_v) {
  auto it = g_blocks.find(handle);
  if (it == g_blocks.end()) {
    set_error("arrow_csr_scale: bad handle");
    return -1;
  }
  const CsrBlock &blk = it->second;
  if (blk.nnz == 0) return 0;
  if (!row_scale_dev && !col_scale0_dev && !col_scale1_dev) return 0;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  return blk.dtype == 64
             ? launch_csr_scale<double>(blk, row_scale_dev, col_scale0_dev,
                                        col_scale1_dev, stream)
             : launch_csr_scale<float>(blk, row_scale_dev, col_scale0_dev,
                                       col_scale1_dev, stream);
}

int arrow_spmm_dual(int64_t handle, const float *X0_dev, const float *X1_dev,
                    float *C_dev, int64_t k, int beta, void *stream_v) {
  return spmm_dual_impl<float>(handle, X0_dev, X1_dev, C_dev, k, beta, stream_v);
}

int arrow_spmm(int64_t handle, const float *X_dev, float *C_dev, int64_t k,
               int beta, void *stream_v) {
  return arrow_spmm_dual(handle, X_dev, X_dev, C_dev, k, beta, stream_v);
}

int arrow_spmm_plan(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                    int n_out) {
  return spmm_plan_export("arrow_spmm_plan", 32, k, nnz, queue_mode, out, n_out);
}

int arrow_spmm_dual_f64(int64_t handle, const double *X0_dev,
                        const double *X1_dev, double *C_dev, int64_t k,
                        int beta, void *stream_v) {
  return spmm_dual_impl<double>(handle, X0_dev, X1_dev, C_dev, k, beta, stream_v);
}

int arrow_spmm_f64(int64_t handle, const double *X_dev, double *C_dev,
                   int64_t k, int beta, void *stream_v) {
  return arrow_spmm_dual_f64(handle, X_dev, X_dev, C_dev, k, beta, stream_v);
}

int arrow_spmm_plan_f64(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                        int n_out) {
  return spmm_plan_export("arrow_spmm_plan_f64", 64, k, nnz, queue_mode, out,
                          n_out);
}

// float64 routing: the pure copies move each row as 2k floats through the
// fp32 kernels (bit-exact, and float4 = two doubles when k is even); the
// two adding forms are the same kernels instantiated for double.
int arrow_permute_rows_f64(double *dst, const double *src,
                           const int64_t *dst_idx, const int64_t *src_idx,
                           int64_t n, int64_t k, void *stream) {
  return launch_permute<float, false>(reinterpret_cast<float *>(dst),
                                      reinterpret_cast<const float *>(src),
                                      dst_idx, src_idx, n, 2 * k,
                                      (hipStream_t)stream);
}

int arrow_permute_add_rows_f64(double *dst, const double *src,
                               const int64_t *dst_idx, const int64_t *src_idx,
                               int64_t n, int64_t k, void *stream) {
  if (n > 0 && !src_idx) {
    set_error("arrow_permute_add_rows_f64: src_idx is NULL");
    return -1;
  }
  return launch_permute<double, true>(dst, src, dst_idx, src_idx, n, k,
                                      (hipStream_t)stream);
}

int arrow_gather_rows_f64(const double *src, double *dst, const int64_t *idx,
                          int64_t n, int64_t k, void *stream) {
  return launch_route<float, RouteOp::Gather>(
      reinterpret_cast<float *>(dst), reinterpret_cast<const float *>(src),
      idx, n, 2 * k, (hipStream_t)stream);
}

int arrow_scatter_rows_f64(double *dst, const double *src, const int64_t *idx,
                           int64_t n, int64_t k, void *stream) {
  return launch_route<float, RouteOp::Scatter>(
      reinterpret_cast<float *>(dst), reinterpret_cast<const float *>(src),
      idx, n, 2 * k, (hipStream_t)stream);
}

int arrow_scatter_add_rows_f64(double *dst, const double *src,
                               const int64_t *idx, int64_t n, int64_t k,
                               void *stream) {
  return launch_route<double, RouteOp::ScatterAdd>(dst, src, idx, n, k,
                                                   (hipStream_t)stream);
}

// bfloat16 features (ABI 1004): raw bf16 bits over a float32 structure.
int arrow_spmm_dual_bf16(int64_t handle, const uint16_t *X0_dev,
                         const uint16_t *X1_dev, uint16_t *C_dev, int64_t k,
                         int beta, void *stream_v) {
  return spmm_dual_impl<uint16_t>(handle, X0_dev, X1_dev, C_dev, k, beta,
                                  stream_v);
}

int arrow_spmm_bf16(int64_t handle, const uint16_t *X_dev, uint16_t *C_dev,
                    int64_t k, int beta, void *stream_v) {
  return arrow_spmm_dual_bf16(handle, X_dev, X_dev, C_dev, k, beta, stream_v);
}

int arrow_spmm_plan_bf16(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                         int n_out) {
  return spmm_plan_export("arrow_spmm_plan_bf16", 16, k, nnz, queue_mode, out,
                          n_out);
}

// Affine step (ABI 1005): C = alpha * (A @ X) + gamma * R + beta * C, fused
// into the write-back of the same launches the plain entry points make.
int arrow_spmm_dual_affine(int64_t handle, const float *X0_dev,
                           const float *X1_dev, float *C_dev,
                           const float *R_dev, int64_t k, double alpha,
                           double gamma, int beta, void *stream) {
  return spmm_affine<float>(handle, X0_dev, X1_dev, C_dev, R_dev, k, alpha,
                            gamma, beta, stream);
}

int arrow_spmm_affine(int64_t handle, const float *X_dev, float *C_dev,
                      const float *R_dev, int64_t k, double alpha,
                      double gamma, int beta, void *stream) {
  return spmm_affine<float>(handle, X_dev, X_dev, C_dev, R_dev, k, alpha,
                            gamma, beta, stream);
}

int arrow_spmm_dual_affine_f64(int64_t handle, const double *X0_dev,
                               const double *X1_dev, double *C_dev,
                               const double *R_dev, int64_t k, double alpha,
                               double gamma, int beta, void *stream) {
  return spmm_affine<double>(handle, X0_dev, X1_dev, C_dev, R_dev, k, alpha,
                             gamma, beta, stream);
}

int arrow_spmm_affine_f64(int64_t handle, const double *X_dev, double *C_dev,
                          const double *R_dev, int64_t k, double alpha,
                          double gamma, int beta, void *stream) {
  return spmm_affine<double>(handle, X_dev, X_dev, C_dev, R_dev, k, alpha,
                             gamma, beta, stream);
}

int arrow_spmm_dual_affine_bf16(int64_t handle, const uint16_t *X0_dev,
                                const uint16_t *X1_dev, uint16_t *C_dev,
                                const uint16_t *R_dev, int64_t k,
                                double alpha, double gamma, int beta,
                                void *stream) {
  return spmm_affine<uint16_t>(handle, X0_dev, X1_dev, C_dev, R_dev, k, alpha,
                               gamma, beta, stream);
}

int arrow_spmm_affine_bf16(int64_t handle, const uint16_t *X_dev,
                           uint16_t *C_dev, const uint16_t *R_dev, int64_t k,
                           double alpha, double gamma, int beta,
                           void *stream) {
  return spmm_affine<uint16_t>(handle, X_dev, X_dev, C_dev, R_dev, k, alpha,
                               gamma, beta, stream);
}

int arrow_axpby_rows_f32(float *C_dev, const float *R_dev, int64_t n,
                         int64_t k, double alpha, double gamma,
                         void *stream) {
  return launch_axpby<float>("arrow_axpby_rows_f32", C_dev, R_dev, n, k,
                             alpha, gamma, (hipStream_t)stream);
}

int arrow_axpby_rows_f64(double *C_dev, const double *R_dev, int64_t n,
                         int64_t k, double alpha, double gamma,
                         void *stream) {
  return launch_axpby<double>("arrow_axpby_rows_f64", C_dev, R_dev, n, k,
                              alpha, gamma, (hipStream_t)stream);
}

int arrow_axpby_rows_bf16(uint16_t *C_dev, const uint16_t *R_dev, int64_t n,
                          int64_t k, double alpha, double gamma,
                          void *stream) {
  if (!bf16_k_ok("arrow_axpby_rows_bf16", k)) return -3;
  return launch_axpby<uint16_t>("arrow_axpby_rows_bf16", C_dev, R_dev, n, k,
                                alpha, gamma, (hipStream_t)stream);
}

// Step norms (ABI 1006): the affine step at beta = 0 that also adds
// sum (c - d)^2 and sum c^2 over every row it writes into acc[0], acc[1].
#define ARROW_AFFINE_NORM(sfx, T)                                             \
  int arrow_spmm_dual_affine_norm##sfx(                                       \
      int64_t handle, const T *X0_dev, const T *X1_dev, T *C_dev,             \
      const T *R_dev, const T *D_dev, double *acc_dev, int64_t k,             \
      double alpha, double gamma, int beta, void *stream) {                   \
    return spmm_affine_norm<T>(handle, X0_dev, X1_dev, C_dev, R_dev, D_dev,   \
                               acc_dev, k, alpha, gamma, beta, stream);       \
  }                                                                           \
  int arrow_spmm_affine_norm##sfx(                                            \
      int64_t handle, const T *X_dev, T *C_dev, const T *R_dev,               \
      const T *D_dev, double *acc_dev, int64_t k, double alpha, double gamma, \
      int beta, void *stream) {                                               \
    return spmm_affine_norm<T>(handle, X_dev, X_dev, C_dev, R_dev, D_dev,     \
                               acc_dev, k, alpha, gamma, beta, stream);       \
  }
ARROW_AFFINE_NORM(, float)
ARROW_AFFINE_NORM(_f64, double)
ARROW_AFFINE_NORM(_bf16, uint16_t)
#undef ARROW_AFFINE_NORM

int arrow_diffnorm_rows_f32(const float *C_dev, const float *D_dev, int64_t n,
                            int64_t k, double *acc_dev, void *stream) {
  return launch_diffnorm<float>("arrow_diffnorm_rows_f32", C_dev, D_dev, n, k,
                                acc_dev, (hipStream_t)stream);
}

int arrow_diffnorm_rows_f64(const double *C_dev, const double *D_dev,
                            int64_t n, int64_t k, double *acc_dev,
                            void *stream) {
  return launch_diffnorm<double>("arrow_diffnorm_rows_f64", C_dev, D_dev, n,
                                 k, acc_dev, (hipStream_t)stream);
}

int arrow_diffnorm_rows_bf16(const uint16_t *C_dev, const uint16_t *D_dev,
                             int64_t n, int64_t k, double *acc_dev,
                             void *stream) {
  if (!bf16_k_ok("arrow_diffnorm_rows_bf16", k)) return -3;
  return launch_diffnorm<uint16_t>("arrow_diffnorm_rows_bf16", C_dev, D_dev,
                                   n, k, acc_dev, (hipStream_t)stream);
}

// bf16 routing: the pure copies move each row as k/2 floats through the fp32
// kernels (bit-exact; float4 = 8 bf16); the two adding forms load 16 bytes
// of each side, add in fp32 and round once.
#define ARROW_BF16_ROUTE_K(who)                                               \
  if (!bf16_k_ok(who, k)) return -3

int arrow_permute_rows_bf16(uint16_t *dst, const uint16_t *src,
                            const int64_t *dst_idx, const int64_t *src_idx,
                            int64_t n, int64_t k, void *stream) {
  ARROW_BF16_ROUTE_K("arrow_permute_rows_bf16");
  return launch_permute<float, false>(reinterpret_cast<float *>(dst),
                                      reinterpret_cast<const float *>(src),
                                      dst_idx, src_idx, n, k / 2,
                                      (hipStream_t)stream);
}

int arrow_permute_add_rows_bf16(uint16_t *dst, const uint16_t *src,
                                const int64_t *dst_idx, const int64_t *src_idx,
                                int64_t n, int64_t k, void *stream) {
  ARROW_BF16_ROUTE_K("arrow_permute_add_rows_bf16");
  if (n > 0 && !src_idx) {
    set_error("arrow_permute_add_rows_bf16: src_idx is NULL");
    return -1;
  }
  return launch_permute<uint16_t, true>(dst, src, dst_idx, src_idx, n, k,
                                        (hipStream_t)stream);
}

int arrow_gather_rows_bf16(const uint16_t *src, uint16_t *dst,
                           const int64_t *idx, int64_t n, int64_t k,
                           void *stream) {
  ARROW_BF16_ROUTE_K("arrow_gather_rows_bf16");
  return launch_route<float, RouteOp::Gather>(
      reinterpret_cast<float *>(dst), reinterpret_cast<const float *>(src),
      idx, n, k / 2, (hipStream_t)stream);
}

int arrow_scatter_rows_bf16(uint16_t *dst, const uint16_t *src,
                            const int64_t *idx, int64_t n, int64_t k,
                            void *stream) {
  ARROW_BF16_ROUTE_K("arrow_scatter_rows_bf16");
  return launch_route<float, RouteOp::Scatter>(
      reinterpret_cast<float *>(dst), reinterpret_cast<const float *>(src),
      idx, n, k / 2, (hipStream_t)stream);
}

int arrow_scatter_add_rows_bf16(uint16_t *dst, const uint16_t *src,
                                const int64_t *idx, int64_t n, int64_t k,
                                void *stream) {
  ARROW_BF16_ROUTE_K("arrow_scatter_add_rows_bf16");
  return launch_route<uint16_t, RouteOp::ScatterAdd>(dst, src, idx, n, k,
                                                     (hipStream_t)stream);
}

int arrow_permute_rows_f32(float *dst, const float *src, const int64_t *dst_idx,
                           const int64_t *src_idx, int64_t n, int64_t k,
                           void *stream) {
  return launch_permute<float, false>(dst, src, dst_idx, src_idx, n, k,
                                      (hipStream_t)stream);
}

int arrow_permute_add_rows_f32(float *dst, const float *src,
                               const int64_t *dst_idx, const int64_t *src_idx,
                               int64_t n, int64_t k, void *stream) {
  return launch_permute<float, true>(dst, src, dst_idx, src_idx, n, k,
                                     (hipStream_t)stream);
}

int arrow_gather_rows_f32(const float *src, float *dst, const int64_t *idx,
                          int64_t n, int64_t k, void *stream) {
  return launch_route<float, RouteOp::Gather>(dst, src, idx, n, k,
                                              (hipStream_t)stream);
}

int arrow_scatter_rows_f32(float *dst, const float *src, const int64_t *idx,
                           int64_t n, int64_t k, void *stream) {
  return launch_route<float, RouteOp::Scatter>(dst, src, idx, n, k,
                                               (hipStream_t)stream);
}

int arrow_scatter_add_rows_f32(float *dst, const float *src, const int64_t *idx,
                               int64_t n, int64_t k, void *stream) {
  return launch_route<float, RouteOp::ScatterAdd>(dst, src, idx, n, k,
                                                  (hipStream_t)stream);
}

}  // extern "C"
