// Bitmap-driven sparse logit edits ahead of the fused samplers.
//
// Repetition penalty and guided-decoding masks are both per-row SETS of token
// ids: "has occurred in prompt + output" and "is allowed next".  Each set is a
// device bitmap, 1 bit per vocab entry:
//
//   uint32 [slots, W]   bit (t & 31) of word (t >> 5) stands for token t
//   W = ceil(V / 32) rounded up to a multiple of 4 (16-byte rows)
//
// At V = 128256 a row is 16 KB, 1/16 of a bf16 logit row, and the bitmaps
// decide which logits are read or written at all.  The unit of work is a
// PIECE of 8 tokens: one bitmap byte, one 16-byte vector of 16-bit logits
// (two for f32).  Lane L of a wave owns piece base + L, so a wave step covers
// 512 tokens with contiguous loads and stores, and reads its seen and allow
// bytes from 16 consecutive words each (word (base + L) >> 2: four lanes share
// a word, which the L1 serves).  Every piece is one of
//
//   skip        nothing seen (or penalty 1.0) and everything allowed: no logit
//               traffic; a ballot lets the whole wave pass over 1 KB of logits
//               (nearly every step of a penalty-only row)
//   store-only  nothing allowed: -inf is stored without a load (the bulk of a
//               guided row)
//   mixed       load, edit the touched elements, store
//
// Per element: a seen token's logit becomes x > 0 ? x / p : x * p in f32,
// rounded once to T (the torch path's formula; -inf from an earlier EOS ban
// stays -inf), then a disallowed token's becomes -inf.  Untouched elements of
// a mixed piece keep their bits.
//
// The grid is (edit row, vocab chunk) over a compact list of edit rows; rows
// not listed are never touched.  All bitmap bytes of a wave's steps are
// fetched before the first logit access, so the dependent logit loads of the
// few touched pieces overlap.  No LDS, no atomics in the edit kernel: each
// element is written by exactly one lane, so results repeat bit-for-bit.
//
// token_bitmap_scatter_kernel ORs (slot, token) pairs into a bitmap with
// global atomicOr: order-independent, duplicates harmless, pairs outside the
// bitmap or the vocab dropped.

#include "common.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE_SIZE;
constexpr int kSteps = 4;        // wave steps per wave: 8192 tokens per block
constexpr int kPieceTokens = 8;  // one bitmap byte
constexpr int kBlockPieces = kWaves * kSteps * WAVE_SIZE;

__global__ __launch_bounds__(kThreads) void token_bitmap_scatter_kernel(
    unsigned* __restrict__ bitmap,   // [nslots, W]
    const int* __restrict__ slots,   // [P]
    const int* __restrict__ tokens,  // [P]
    const int P, const int nslots, const int W, const int V) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P) return;
  const int s = slots[i];
  const int t = tokens[i];
  if (s < 0 || s >= nslots || t < 0 || t >= V) return;
  atomicOr(&bitmap[(long)s * W + (t >> 5)], 1u << (t & 31));
}

// The 8 logits of one piece: 16-byte vectors, one for 16-bit T, two for f32.
template <typename T>
struct Piece {
  static constexpr int kVecs = kPieceTokens / Vec16<T>::kElems;
  Vec16<T> v[kVecs];
};

template <typename T>
DEVINLINE Piece<T> load_piece(const T* p) {
  Piece<T> r;
#pragma unroll
  for (int i = 0; i < Piece<T>::kVecs; ++i)
    r.v[i] = load16(p + i * Vec16<T>::kElems);
  return r;
}

template <typename T>
DEVINLINE void store_piece(T* p, const Piece<T>& r) {
#pragma unroll
  for (int i = 0; i < Piece<T>::kVecs; ++i)
    store16(p + i * Vec16<T>::kElems, r.v[i]);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void logits_edit_kernel(
    T* __restrict__ logits,               // [N, V], edited in place
    const int* __restrict__ rows,         // [E] logit row of each edit row
    const float* __restrict__ penalties,  // [E] 1.0 = none
    const unsigned* __restrict__ seen,    // [n_seen, W] or null
    const int* __restrict__ seen_slots,   // [E] -1 = none
    const unsigned* __restrict__ allow,   // [n_allow, W] or null
    const int* __restrict__ allow_slots,  // [E] -1 = none
    const int N, const int V, const int W, const int n_seen,
    const int n_allow) {
  constexpr int kE = Vec16<T>::kElems;
  const int e = blockIdx.x;
  const int row = rows[e];
  if (row < 0 || row >= N) return;
  const float pen = penalties[e];
  const int ss = seen ? seen_slots[e] : -1;
  const int as = allow ? allow_slots[e] : -1;
  // block-uniform: which bitmaps this row consults at all
  const unsigned* srow =
      (pen != 1.f && ss >= 0 && ss < n_seen) ? seen + (long)ss * W : nullptr;
  const unsigned* arow =
      (as >= 0 && as < n_allow) ? allow + (long)as * W : nullptr;
  if (!srow && !arow) return;

  T* lrow = logits + (long)row * V;
  const int npieces = V / kPieceTokens;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  // the block's waves interleave their steps: step s of wave w is wave step
  // blockIdx.y * kWaves * kSteps + s * kWaves + w of the row
  const int piece0 = (blockIdx.y * kWaves * kSteps + wave) * WAVE_SIZE + lane;

  unsigned sb[kSteps], ab[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int piece = piece0 + s * kWaves * WAVE_SIZE;
    sb[s] = 0u;
    ab[s] = 0xFFu;  // pieces past the row: skip
    if (piece < npieces) {
      const int word = piece >> 2;
      const int sh = (piece & 3) * 8;
      if (srow) sb[s] = (srow[word] >> sh) & 0xFFu;
      if (arow) ab[s] = (arow[word] >> sh) & 0xFFu;
    }
  }

  const T ninf = ScalarOps<T>::from_f32(-INFINITY);
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const bool touch = sb[s] != 0u || ab[s] != 0xFFu;
    if (__ballot(touch) == 0ull) continue;  // wave-uniform: 1 KB untouched
    if (!touch) continue;
    T* p = lrow + (long)(piece0 + s * kWaves * WAVE_SIZE) * kPieceTokens;
    Piece<T> x;
    if (ab[s] == 0u) {
#pragma unroll
      for (int i = 0; i < kPieceTokens; ++i) x.v[i / kE].data[i % kE] = ninf;
    } else {
      x = load_piece(p);
#pragma unroll
      for (int i = 0; i < kPieceTokens; ++i) {
        T& el = x.v[i / kE].data[i % kE];
        if (!((ab[s] >> i) & 1u)) {
          el = ninf;
        } else if ((sb[s] >> i) & 1u) {
          const float f = ScalarOps<T>::to_f32(el);
          el = ScalarOps<T>::from_f32(f > 0.f ? f / pen : f * pen);
        }
      }
    }
    store_piece(p, x);
  }
}

}  // namespace

void launch_token_bitmap_scatter(unsigned* bitmap, const int* slots,
                                 const int* tokens, int P, int nslots, int W,
                                 int V, hipStream_t stream) {
  hipLaunchKernelGGL(token_bitmap_scatter_kernel,
                     dim3((P + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, bitmap, slots, tokens, P, nslots, W, V);
}

template <typename T>
void launch_logits_edit(T* logits, const int* rows, const float* penalties,
                        const unsigned* seen, const int* seen_slots,
                        const unsigned* allow, const int* allow_slots, int E,
                        int N, int V, int W, int n_seen, int n_allow,
                        hipStream_t stream) {
  const int npieces = V / kPieceTokens;
  const dim3 grid(E, (npieces + kBlockPieces - 1) / kBlockPieces);
  hipLaunchKernelGGL(logits_edit_kernel<T>, grid, dim3(kThreads), 0, stream,
                     logits, rows, penalties, seen, seen_slots, allow,
                     allow_slots, N, V, W, n_seen, n_allow);
}

#define INSTANTIATE_LOGITS_EDIT(T)                                           \
  template void launch_logits_edit<T>(T*, const int*, const float*,          \
                                      const unsigned*, const int*,           \
                                      const unsigned*, const int*, int, int, \
                                      int, int, int, int, hipStream_t);

INSTANTIATE_LOGITS_EDIT(__hip_bfloat16)
INSTANTIATE_LOGITS_EDIT(__half)
INSTANTIATE_LOGITS_EDIT(float)
