// Segmented multi-LoRA (SGMV) shrink/expand on MFMA for prefill-sized batches
// (SURVEY.md E12).  Same contract as lora_bgmv.hip — per-token adapter slot
// (-1 = none), rank-padded stacks A_stack [L, R, K] / B_stack [L, N, R],
//   out[t, off:off+N] += scale[s] · B[s] · (A[s] · x[t])   in place —
// but bf16 only and built for T in the hundreds to thousands, where BGMV's
// one-workgroup-per-token VALU dots re-read A and B per token and leave the
// matrix units idle.
//
// Segments without a sort.  Tokens of one prefill sequence are contiguous, so
// nearly every 32-token tile is one adapter.  Each wave reads its tile's
// slots and peels off distinct values (first remaining row's slot, ballot for
// membership); per distinct slot it runs the MFMA product for the whole tile
// and keeps the rows that belong to it.  Uniform tile = one pass, a sequence
// boundary = two, a decode-like tile degrades to one pass per adapter but
// stays correct.  No host sort, nonzero() or sync; launch geometry depends on
// shapes only (hipGraph-safe).
//
// shrink  tmp[split, t, r] = sum_k x[t, k] · A[slot(t)][r, k]
//   v_mfma_f32_16x16x32_bf16, x tile as the A operand (two 16-token
//   m-blocks), A_stack rows as the B operand (ceil(R/16) n-blocks).  Both are
//   K-contiguous, so a lane's fragment (row lane&15, 8 k at (lane>>4)*8) is
//   one 16-byte global load — no LDS staging for layout.  SG_KU k-steps of
//   loads are issued ahead of the MFMAs that consume them.  The grid splits K
//   (lora_sgmv_num_ksplit, shape-pure) and the 4 waves of a workgroup split
//   their share again, folded through LDS in wave order.  Each grid split
//   writes its own f32 partial; no atomics, so results repeat bit-for-bit.
//
// expand  out[t, off+n] += scale[s] · sum_r B[s][n, r] · tmp[t, r]
//   Swapped operands: B_stack rows are the A operand (n along M), tmp^T the
//   B operand, so a lane's accumulator registers are consecutive n of ONE
//   token.  The wave sums the K-split partials in order and splits each f32
//   into bf16 hi + bf16 lo = bf16(v - hi); hi·B + lo·B keeps tmp accurate to
//   ~2^-16 like BGMV's f32 tmp, so crossing the dispatch threshold moves
//   results by at most the final rounding.  n-blocks go in pairs whose rows
//   are interleaved (block h row m -> n = (m>>2)*8 + h*4 + (m&3)) so a lane
//   ends up with 8 consecutive n: one 16-byte read-modify-write of out,
//   acc·scale + out in f32, one rounding.

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

namespace {

constexpr int SG_TOK = 32;    // tokens per tile: two 16-row m-blocks
constexpr int SG_WAVES = 4;   // waves per workgroup
constexpr int SG_KU = 4;      // shrink: k-steps of loads in flight
constexpr int SG_NW = 128;    // expand: output columns per wave (4 n-pairs)
constexpr int SG_MIN_KDEPTH = 512;  // shrink: least k per workgroup

DEVINLINE bf16x8_t sg_load8(const __hip_bfloat16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

// Slot of tile row `lane` (lanes >= SG_TOK, rows past T and ids outside
// [0, L) read as -1, so nothing downstream indexes a stack with them).
DEVINLINE int sg_tile_slot(const int* __restrict__ slots, int t0, int T, int L,
                           int lane) {
  int s = -1;
  if (lane < SG_TOK && t0 + lane < T) s = slots[t0 + lane];
  return (s >= 0 && s < L) ? s : -1;
}

// Peel the next distinct adapter off the tile: returns its slot (wave
// uniform), sets `members` to the tile rows that carry it.
DEVINLINE int sg_next_slot(int slot, unsigned long long& remaining,
                           unsigned long long& members) {
  const int first = __builtin_ctzll(remaining);
  const int s = __builtin_amdgcn_readfirstlane(__shfl(slot, first, WAVE_SIZE));
  members = __ballot(slot == s);
  remaining &= ~members;
  return s;
}

// 8 r-consecutive elements of a B_stack row from r0, zero past R.  Rows are
// only 16-byte aligned when R % 8 == 0; other ranks take the scalar loop.
DEVINLINE bf16x8_t sg_load_b(const __hip_bfloat16* __restrict__ b_row, int r0,
                             int R) {
  bf16x8_t v = {};
  if ((R & 7) == 0) {
    if (r0 < R) v = sg_load8(b_row + r0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (r0 + j < R) v[j] = __builtin_bit_cast(short, b_row[r0 + j]);
  }
  return v;
}

}  // namespace

// ---------------------------------------------------------------------------
// shrink.  grid (ceil(T/32), S), block 256; NB = ceil(R/16).
// ---------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(256) void lora_sgmv_shrink_kernel(
    float* __restrict__ tmp,                    // [S, T, NB*16]
    const __hip_bfloat16* __restrict__ x,       // [T, K]
    const __hip_bfloat16* __restrict__ a_stack,  // [L, R, K]
    const int* __restrict__ slots,              // [T]
    const int T, const int R, const int K, const int L) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;
  const int quad = lane >> 4;
  const int t0 = blockIdx.x * SG_TOK;
  const int k_wave = K / (int)gridDim.y / SG_WAVES;  // multiple of 32
  const int k_lo = ((int)blockIdx.y * SG_WAVES + wave) * k_wave;
  const int k_hi = k_lo + k_wave;

  const int slot = sg_tile_slot(slots, t0, T, L, lane);
  unsigned long long remaining = __ballot(slot >= 0);

  // rows past T read row T-1: their accumulator rows are never stored
  const __hip_bfloat16* x_row[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
    x_row[mb] = x + (long)min(t0 + mb * 16 + row, T - 1) * K + quad * 8;

  __shared__ f32x4_t red[(SG_WAVES - 1) * 2 * NB * 64];

  while (remaining) {
    unsigned long long members;
    const int s = sg_next_slot(slot, remaining, members);

    const __hip_bfloat16* a_row[NB];
    bool a_ok[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int r = nb * 16 + row;
      a_ok[nb] = r < R;  // rank padding up to NB*16 is zero-filled, not read
      a_row[nb] = a_stack + ((long)s * R + min(r, R - 1)) * K + quad * 8;
    }

    f32x4_t acc[2][NB];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int k = k_lo; k < k_hi; k += 32 * SG_KU) {
      bf16x8_t xf[SG_KU][2], af[SG_KU][NB];
#pragma unroll
      for (int u = 0; u < SG_KU; ++u) {
        // steps past the wave's range re-read k_lo and are zeroed
        const bool k_ok = k + 32 * u < k_hi;
        const int kk = k_ok ? k + 32 * u : k_lo;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          xf[u][mb] = sg_load8(x_row[mb] + kk);
          if (!k_ok) xf[u][mb] = bf16x8_t{};
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          af[u][nb] = sg_load8(a_row[nb] + kk);
          if (!(k_ok && a_ok[nb])) af[u][nb] = bf16x8_t{};
        }
      }
#pragma unroll
      for (int u = 0; u < SG_KU; ++u)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xf[u][mb], af[u][nb], acc[mb][nb], 0, 0, 0);
    }

    // fold the workgroup's four k-ranges in wave order; wave 0 stores.  The
    // pass count is the same for every wave (same tile), so the barriers are
    // uniform.
    if (wave > 0) {
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          red[(((wave - 1) * 2 + mb) * NB + nb) * 64 + lane] = acc[mb][nb];
    }
    __syncthreads();
    if (wave == 0) {
      float* tmp_split = tmp + (long)blockIdx.y * T * (NB * 16);
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          f32x4_t v = acc[mb][nb];
#pragma unroll
          for (int w = 0; w < SG_WAVES - 1; ++w)
            v += red[((w * 2 + mb) * NB + nb) * 64 + lane];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int trow = mb * 16 + quad * 4 + reg;  // D row = token
            if ((members >> trow) & 1)
              tmp_split[(long)(t0 + trow) * (NB * 16) + nb * 16 + row] = v[reg];
          }
        }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// expand.  grid (ceil(T/32), ceil(N/512)), block 256; KS = ceil(Rpad/32).
// No LDS, no barriers: waves leave independently.
// ---------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void lora_sgmv_expand_kernel(
    __hip_bfloat16* __restrict__ out,            // [T, out_w]
    const float* __restrict__ tmp,               // [S, T, Rpad]
    const __hip_bfloat16* __restrict__ b_stack,  // [L, N, R]
    const int* __restrict__ slots,               // [T]
    const float* __restrict__ scales,            // [L]
    const int T, const int R, const int Rpad, const int N, const int out_w,
    const int off, const int S, const int L) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;
  const int quad = lane >> 4;
  const int t0 = blockIdx.x * SG_TOK;
  const int n_wave = ((int)blockIdx.y * SG_WAVES + wave) * SG_NW;
  if (n_wave >= N) return;

  const int slot = sg_tile_slot(slots, t0, T, L, lane);
  unsigned long long remaining = __ballot(slot >= 0);
  if (!remaining) return;

  // D column = token: this lane's token in each 16-token block
  int my_slot[2];
#pragma unroll
  for (int tb = 0; tb < 2; ++tb)
    my_slot[tb] = __shfl(slot, tb * 16 + row, WAVE_SIZE);

  // tmp^T fragments: partials summed in split order, then hi/lo bf16
  bf16x8_t hi[2][KS], lo[2][KS];
#pragma unroll
  for (int tb = 0; tb < 2; ++tb) {
    const int t = min(t0 + tb * 16 + row, T - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int r0 = ks * 32 + quad * 8;
      // shrink leaves rows without an adapter unwritten: zero, not read
      const bool ok = r0 < Rpad && my_slot[tb] >= 0;
      const float* p = tmp + (long)t * Rpad + (r0 < Rpad ? r0 : 0);
      f32x4_t v[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
      for (int sp = 0; sp < S; ++sp) {
        const f32x4_t* q =
            reinterpret_cast<const f32x4_t*>(p + (long)sp * T * Rpad);
        v[0] += q[0];
        v[1] += q[1];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = ok ? v[j >> 2][j & 3] : 0.f;
        const __hip_bfloat16 h = __float2bfloat16(f);
        const __hip_bfloat16 l = __float2bfloat16(f - __bfloat162float(h));
        hi[tb][ks][j] = __builtin_bit_cast(short, h);
        lo[tb][ks][j] = __builtin_bit_cast(short, l);
      }
    }
  }

  while (remaining) {
    unsigned long long members;
    const int s = sg_next_slot(slot, remaining, members);
    const float scale = scales[s];
    const __hip_bfloat16* b_s = b_stack + (long)s * N * R;

    for (int nb = n_wave; nb < min(n_wave + SG_NW, N); nb += 32) {
      // this lane's 8 output columns of each of its two tokens
      bool mine[2];
      __hip_bfloat16* o_ptr[2];
      Vec16<__hip_bfloat16> ov[2];
#pragma unroll
      for (int tb = 0; tb < 2; ++tb) {
        mine[tb] = my_slot[tb] == s;  // implies token < T
        o_ptr[tb] = out + (long)(t0 + tb * 16 + row) * out_w + off + nb + quad * 8;
        if (mine[tb]) ov[tb] = load16(o_ptr[tb]);
      }

      f32x4_t acc[2][2];  // [n half][token block]
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = nb + (row >> 2) * 8 + h * 4 + (row & 3);
        bf16x8_t bf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          bf[ks] = sg_load_b(b_s + (long)n * R, ks * 32 + quad * 8, R);
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
          acc[h][tb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            acc[h][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bf[ks], hi[tb][ks], acc[h][tb], 0, 0, 0);
            acc[h][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bf[ks], lo[tb][ks], acc[h][tb], 0, 0, 0);
          }
        }
      }

#pragma unroll
      for (int tb = 0; tb < 2; ++tb) {
        if (!mine[tb]) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          ov[tb].data[j] = __float2bfloat16(
              acc[j >> 2][tb][j & 3] * scale + __bfloat162float(ov[tb].data[j]));
        store16(o_ptr[tb], ov[tb]);
      }
    }
  }
}

// K-split of the shrink grid: a pure function of shapes (capture-safe).
// Doubles while the grid is under 512 workgroups, every workgroup keeps at
// least SG_MIN_KDEPTH of k and its four waves get whole 32-k steps.
int lora_sgmv_num_ksplit(int T, int K) {
  const int tiles = (T + SG_TOK - 1) / SG_TOK;
  int ks = 1;
  while (ks < 16 && tiles * ks * 2 <= 512 &&
         (K / (ks * 2)) % (32 * SG_WAVES) == 0 &&
         K / (ks * 2) >= SG_MIN_KDEPTH)
    ks *= 2;
  return ks;
}

void launch_lora_sgmv_shrink(float* tmp, const __hip_bfloat16* x,
                             const __hip_bfloat16* a_stack, const int* slots,
                             int T, int R, int K, int L, int S,
                             hipStream_t stream) {
  const dim3 grid((T + SG_TOK - 1) / SG_TOK, S);
#define SG_SHRINK(NB)                                                        \
  hipLaunchKernelGGL(lora_sgmv_shrink_kernel<NB>, grid, dim3(64 * SG_WAVES), \
                     0, stream, tmp, x, a_stack, slots, T, R, K, L)
  switch ((R + 15) / 16) {
    case 1: SG_SHRINK(1); break;
    case 2: SG_SHRINK(2); break;
    case 3: SG_SHRINK(3); break;
    default: SG_SHRINK(4); break;
  }
#undef SG_SHRINK
}

void launch_lora_sgmv_expand(__hip_bfloat16* out, const float* tmp,
                             const __hip_bfloat16* b_stack, const int* slots,
                             const float* scales, int T, int R, int N,
                             int out_w, int off, int L, int S,
                             hipStream_t stream) {
  const int Rpad = (R + 15) / 16 * 16;
  const dim3 grid((T + SG_TOK - 1) / SG_TOK,
                  (N + SG_NW * SG_WAVES - 1) / (SG_NW * SG_WAVES));
#define SG_EXPAND(KS)                                                        \
  hipLaunchKernelGGL(lora_sgmv_expand_kernel<KS>, grid, dim3(64 * SG_WAVES), \
                     0, stream, out, tmp, b_stack, slots, scales, T, R, Rpad,  \
                     N, out_w, off, S, L)
  if (Rpad <= 32) SG_EXPAND(1);
  else SG_EXPAND(2);
#undef SG_EXPAND
}
