// MoE routing, dispatch and combine: everything between the
// router GEMM and the all-reduce that is not the grouped GEMM itself.
//
//   route     weights[t, :], ids[t, :] = top-k of the router logits (selected
//             on the logits, ties to the lower expert), softmax over the k
//             selected logits in f32 (== softmax over all E, renormalised)
//   dispatch  stable counting sort of the (token, slot) pairs by expert, then
//             token, then slot:  seg_off [E+1] (what moe_gemm takes),
//             src_row [T*k] (token of each sorted position, what the
//             gathering moe_gemm takes) and pos [T, k] (sorted position of
//             each pair, what the combine takes)
//   combine   out[t, :] = bf16(sum_j weights[t, j] * ye[pos[t, j], :]), f32
//             accumulation in slot order, one rounding
//
// Design.  A workgroup of 256 threads owns a fixed block of 256 tokens.  A
// group of G = 1/2/4/8 adjacent lanes (template, E <= 8*G) holds one token's
// row, 8 logits per lane in registers (one 16-byte load for 16-bit logits),
// and the block takes its tokens in G passes of 256/G.  Top-k is k rounds of
// argmax: a statically unrolled scan of the lane's 8 registers under a
// `taken` bitmask, then a xor-butterfly over the G lanes on (value, index)
// with the lower index winning ties; lane 0's winner is broadcast so every
// lane of the group retires the same expert and the k ids are distinct by
// construction.  The chosen ids go to LDS as one packed byte string per token.
//
// Ranking does not peel distinct values as lora_sgmv does: a token names an
// expert at most once, so for one expert a 64-token wave tile is a single
// ballot, a pair's rank inside the block is the running count plus the
// popcount of the lower lanes, and the wave's final count is the block's
// histogram entry.  The four waves split the experts.  No atomics anywhere,
// so every position is a pure function of the logits.
//
// T <= 256 (every decode step): the one block scans its own histogram into
// seg_off and writes src_row / pos itself — one launch.  Larger T: blocks
// leave their histogram in hist[nblk, E] and block-local ranks in pos, and a
// second small kernel (same grid) adds seg_off[e] + the counts of the blocks
// before it.  The launch count depends on T alone.

#include "common.h"

#include <climits>

#define MD_BLOCK_TOKENS 256
#define MD_THREADS 256

typedef unsigned long long md_u64;

// 8 consecutive logits of one row starting at expert e0, as f32; experts past
// E read as 0 and are masked by the caller
template <typename T>
DEVINLINE void md_load8(const T* __restrict__ row, int e0, int E, bool vec,
                        float v[8]) {
  if (vec && e0 + 8 <= E) {
    if constexpr (sizeof(T) == 2) {
      const Vec16<T> a = load16(row + e0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ScalarOps<T>::to_f32(a.data[j]);
    } else {
      const Vec16<T> a = load16(row + e0);
      const Vec16<T> b = load16(row + e0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = ScalarOps<T>::to_f32(a.data[j]);
        v[4 + j] = ScalarOps<T>::to_f32(b.data[j]);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = e0 + j < E ? ScalarOps<T>::to_f32(row[e0 + j]) : 0.f;
  }
}

// inclusive scan over the wave
DEVINLINE int md_wave_scan(int x, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const int o = __shfl_up(x, off, WAVE_SIZE);
    if (lane >= off) x += o;
  }
  return x;
}

template <typename T, int G>
__global__ __launch_bounds__(MD_THREADS) void moe_route_dispatch_kernel(
    float* __restrict__ weights,   // [T, k]
    int* __restrict__ ids,         // [T, k]
    int* __restrict__ seg_off,     // [E+1]         (written when gridDim.x == 1)
    int* __restrict__ src_row,     // [T*k]         (written when gridDim.x == 1)
    int* __restrict__ pos,         // [T, k]        (block-local rank otherwise)
    int* __restrict__ hist,        // [nblk, E]     (written when gridDim.x > 1)
    const T* __restrict__ logits,  // [T, E]
    const int Tn, const int E, const int k, const int vec,
    const int route_only) {
  __shared__ md_u64 s_ids[MD_BLOCK_TOKENS];  // byte j = expert of slot j, 0xFF = none
  __shared__ unsigned short s_rank[MD_BLOCK_TOKENS * 8];
  __shared__ int s_hist[64];
  __shared__ int s_base[64];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int g = tid % G;
  const int e0 = g * 8;
  const int t0 = blockIdx.x * MD_BLOCK_TOKENS;

  // ---- route: G passes of 256/G tokens ---------------------------------
  for (int pass = 0; pass < G; ++pass) {
    const int tl = pass * (MD_THREADS / G) + tid / G;
    const int t = t0 + tl;
    const bool valid = t < Tn;  // uniform over the lane group

    float v[8];
    if (valid) {
      md_load8<T>(logits + (long)t * E, e0, E, vec != 0, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    unsigned taken = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (e0 + j >= E) taken |= 1u << j;

    float selv[8];
    int seli[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      selv[r] = 0.f;
      seli[r] = 0;
      if (r < k) {  // k is uniform over the grid
        float bv = 0.f;
        int bi = INT_MAX;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!((taken >> j) & 1u) && (bi == INT_MAX || v[j] > bv)) {
            bv = v[j];
            bi = e0 + j;
          }
        if (G > 1) {
#pragma unroll
          for (int off = G / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, WAVE_SIZE);
            const int oi = __shfl_xor(bi, off, WAVE_SIZE);
            if (oi != INT_MAX &&
                (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
              bv = ov;
              bi = oi;
            }
          }
          // one winner for the whole group, whatever a NaN did to the order
          bv = __shfl(bv, lane - g, WAVE_SIZE);
          bi = __shfl(bi, lane - g, WAVE_SIZE);
        }
        selv[r] = bv;
        seli[r] = bi;
        if ((bi >> 3) == g) taken |= 1u << (bi & 7);
      }
    }

    if (g == 0) {
      md_u64 packed = ~0ull;
      if (valid) {
        float ex[8];
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (r < k) {
            ex[r] = __expf(selv[r] - selv[0]);
            sum += ex[r];
          }
        const float inv = 1.f / sum;
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (r < k) {
            weights[(long)t * k + r] = ex[r] * inv;
            ids[(long)t * k + r] = seli[r];
            packed = (packed & ~(0xFFull << (8 * r))) |
                     ((md_u64)seli[r] << (8 * r));
          }
      }
      s_ids[tl] = packed;
    }
  }
  if (route_only) return;
  __syncthreads();

  // ---- rank: per expert, one ballot per 64-token tile --------------------
  for (int e = wave; e < E; e += MD_THREADS / WAVE_SIZE) {
    int run = 0;
#pragma unroll
    for (int tile = 0; tile < MD_BLOCK_TOKENS / WAVE_SIZE; ++tile) {
      const int tl = tile * WAVE_SIZE + lane;
      const md_u64 pk = s_ids[tl];
      int slot = -1;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if ((int)((pk >> (8 * j)) & 0xFF) == e) slot = j;
      const md_u64 members = __ballot(slot >= 0);
      if (slot >= 0)
        s_rank[tl * 8 + slot] =
            (unsigned short)(run + __popcll(members & ((1ull << lane) - 1)));
      run += __popcll(members);
    }
    if (lane == 0) s_hist[e] = run;
  }
  __syncthreads();

  // ---- place --------------------------------------------------------------
  const bool single = gridDim.x == 1;
  if (single) {
    if (wave == 0) {
      const int c = lane < E ? s_hist[lane] : 0;
      const int incl = md_wave_scan(c, lane);
      if (lane < E) {
        s_base[lane] = incl - c;
        seg_off[lane + 1] = incl;
      }
      if (lane == 0) seg_off[0] = 0;
    }
    __syncthreads();
  } else if (tid < E) {
    hist[(long)blockIdx.x * E + tid] = s_hist[tid];
  }
  for (int idx = tid; idx < MD_BLOCK_TOKENS * 8; idx += MD_THREADS) {
    const int tl = idx >> 3;
    const int j = idx & 7;
    const int e = (int)((s_ids[tl] >> (8 * j)) & 0xFF);
    if (e == 0xFF) continue;
    const int t = t0 + tl;
    const int r = s_rank[idx];
    if (single) {
      const int p = s_base[e] + r;
      pos[(long)t * k + j] = p;
      src_row[p] = t;
    } else {
      pos[(long)t * k + j] = r;
    }
  }
}

// Second stage for T > 256: same grid as the first.  Every block sums the
// histogram column of each expert (all blocks for seg_off, the blocks before
// it for its own base) and moves its pairs from block-local rank to position.
__global__ __launch_bounds__(MD_THREADS) void moe_dispatch_place_kernel(
    int* __restrict__ seg_off, int* __restrict__ src_row,
    int* __restrict__ pos, const int* __restrict__ ids,
    const int* __restrict__ hist, const int Tn, const int E, const int k) {
  __shared__ int s_base[64];
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  const int nblk = gridDim.x;
  if (tid < WAVE_SIZE) {
    int before = 0, total = 0;
    if (tid < E)
      for (int b = 0; b < nblk; ++b) {
        const int c = hist[(long)b * E + tid];
        total += c;
        if (b < blk) before += c;
      }
    const int incl = md_wave_scan(total, tid);
    if (tid < E) {
      s_base[tid] = incl - total + before;
      if (blk == 0) seg_off[tid + 1] = incl;
    }
    if (blk == 0 && tid == 0) seg_off[0] = 0;
  }
  __syncthreads();
  const long t0 = (long)blk * MD_BLOCK_TOKENS;
  const int npairs = (int)min((long)MD_BLOCK_TOKENS, Tn - t0) * k;
  for (int idx = tid; idx < npairs; idx += MD_THREADS) {
    const long i = t0 * k + idx;
    const int p = s_base[ids[i]] + pos[i];
    pos[i] = p;
    src_row[p] = (int)(t0 + idx / k);
  }
}

// One thread per 16-byte piece of an output row, so a workgroup covers one
// token's 2048 columns or several tokens at smaller H.
__global__ __launch_bounds__(256) void moe_combine_kernel(
    __hip_bfloat16* __restrict__ out,       // [T, H]
    const __hip_bfloat16* __restrict__ ye,  // [T*k, H] sorted rows
    const int* __restrict__ pos,            // [T, k]
    const float* __restrict__ weights,      // [T, k]
    const long n_items, const int H, const int k) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= n_items) return;
  const int hv = H / 8;
  const long t = item / hv;
  const int col = (int)(item % hv) * 8;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int j = 0; j < k; ++j) {
    const float w = weights[t * k + j];
    const Vec16<__hip_bfloat16> v = load16(ye + (long)pos[t * k + j] * H + col);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      acc[i] = fmaf(w, __bfloat162float(v.data[i]), acc[i]);
  }
  Vec16<__hip_bfloat16> o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.data[i] = __float2bfloat16(acc[i]);
  store16(out + t * H + col, o);
}

int moe_dispatch_block_tokens() { return MD_BLOCK_TOKENS; }

template <typename T>
void launch_moe_dispatch(float* weights, int* ids, int* seg_off, int* src_row,
                         int* pos, int* hist, const T* logits, int Tn, int E,
                         int k, bool vec, bool route_only,
                         hipStream_t stream) {
  const int nblk = (Tn + MD_BLOCK_TOKENS - 1) / MD_BLOCK_TOKENS;
  dim3 grid(nblk), block(MD_THREADS);
#define MD_LAUNCH(G)                                                        \
  hipLaunchKernelGGL((moe_route_dispatch_kernel<T, G>), grid, block, 0,     \
                     stream, weights, ids, seg_off, src_row, pos, hist,     \
                     logits, Tn, E, k, (int)vec, (int)route_only)
  if (E <= 8) MD_LAUNCH(1);
  else if (E <= 16) MD_LAUNCH(2);
  else if (E <= 32) MD_LAUNCH(4);
  else MD_LAUNCH(8);
#undef MD_LAUNCH
  if (nblk > 1 && !route_only)
    hipLaunchKernelGGL(moe_dispatch_place_kernel, grid, block, 0, stream,
                       seg_off, src_row, pos, ids, hist, Tn, E, k);
}

template void launch_moe_dispatch<float>(float*, int*, int*, int*, int*, int*,
                                         const float*, int, int, int, bool,
                                         bool, hipStream_t);
template void launch_moe_dispatch<__hip_bfloat16>(float*, int*, int*, int*,
                                                  int*, int*,
                                                  const __hip_bfloat16*, int,
                                                  int, int, bool, bool,
                                                  hipStream_t);
template void launch_moe_dispatch<__half>(float*, int*, int*, int*, int*, int*,
                                          const __half*, int, int, int, bool,
                                          bool, hipStream_t);

void launch_moe_combine(__hip_bfloat16* out, const __hip_bfloat16* ye,
                        const int* pos, const float* weights, int Tn, int H,
                        int k, hipStream_t stream) {
  const long n_items = (long)Tn * (H / 8);
  dim3 grid((unsigned)((n_items + 255) / 256)), block(256);
  hipLaunchKernelGGL(moe_combine_kernel, grid, block, 0, stream, out, ye, pos,
                     weights, n_items, H, k);
}
