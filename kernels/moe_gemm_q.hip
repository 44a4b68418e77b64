// Grouped MoE GEMM on weight-only-quantized expert weights (SURVEY.md E16 /
// E18): moe_gemm_kernel's contract with the experts stored as int8 or packed
// int4-g128, dequantised on the way into LDS.
//
//   h[r, :] = silu(x[r]·dq(Wg_e)^T) * (x[r]·dq(Wu_e)^T)   (gated, [E, 2N, K])
//   y[r, :] = h[r]·dq(W2_e)^T                              (plain, [E, N, K])
// where e = the expert owning sorted row r (seg_off[e] <= r < seg_off[e+1]);
// GATHER reads row r from x[src_row[r]].
//
// Storage is ops.quantize_weight's, stacked per expert: int8 wq [E, rows, K]
// with scales [E, rows]; int4 wq [E, rows, K/2] offset-binary nibbles (even k
// low) with scales [E, rows, K/128].  Flattened to [E*rows, ...] it is the
// 2-D format of gemm_tile_q.hip, so dequant_weight_kernel serves it as is.
//
// Geometry: grid (N/128, E * MBLK), MBLK = ceil(R / BM), expert fastest in
// grid.y.  Each workgroup
// reads its expert's segment bounds itself and exits when its m-chunk lies
// past the end: no host sync, no atomics, and BM / MBLK depend on (R, E)
// alone, so the launch is hipGraph-stable and the result bit-repeatable.
//
// Tile: BM x 128(N) x 64(K) per 4-wave workgroup on
// v_mfma_f32_16x16x32_bf16; wave w owns the W rows [32w, 32w+32) of the
// n-tile against all BM x rows.  The gated kernel stages two W images per
// buffer (gate and up rows of the same n-tile) and keeps two accumulator
// sets.  The conversion work of a slab is 128 x 64 per image whatever BM is:
//   BM = 32  decode-sized segments.  LDS 2 x (16 | 32) KB W + 2 x 4 KB x =
//            40 KB plain / 72 KB gated: 2+ workgroups per CU (160 KB), which
//            is what keeps enough packed bytes in flight to stream the
//            weights.
//   BM = 128 long segments, where re-streaming and re-converting the W tile
//            per 32-row chunk would dominate.  64 KB plain / 96 KB gated.
// moe_gemm_q_block_m picks 128 once the mean segment exceeds 32 rows.
//
// W path: each lane fetches 16 packed bytes per vector (32 int4 / 16 int8
// weights) into registers ahead of use, so the loads fly under the MFMAs:
// one slab ahead in the 128-row tile, two (two register stages) in the
// 32-row tile.  (A packed slab is a half / a quarter of the bf16 kernel's,
// and at decode sizes a few hundred workgroups are all there is: one slab
// ahead left too few bytes in flight there, profiles/r09_moe_gemm_q.txt.)
// The int4 group scale is one more independent load of that stage (a 64-k
// slab never straddles a 128-k group), the int8 row scale is loaded once.
// When a slab's turn comes its registers go through quant_cvt.h's routines
// into the bf16 LDS image: the effective weights are bit-identical to
// ops.dequantize_weight.  x takes the same register route
// (16 B per lane, 8 lanes per row); rows past the segment end are read from
// the segment's last row (in bounds) and their results are never written.
// Both images carry gemm_tile.hip's row>>1 slot skew.

#include "quant_cvt.h"

// QBITS: 8 or 4.  BM: 32 or 128 x rows per workgroup.
template <int QBITS, bool GATED, bool GATHER, int BM>
__global__ __launch_bounds__(256, (GATED && BM == 128) ? 1 : 2)
void moe_gemm_q_kernel(
    __hip_bfloat16* __restrict__ y,        // [R, N]
    const __hip_bfloat16* __restrict__ x,  // [R, K] sorted by expert; GATHER:
                                           // unsorted, row r is x[src_row[r]]
    const unsigned char* __restrict__ wq,  // [E, W_ROWS, K * QBITS / 8]
    const float* __restrict__ wscale,      // [E, W_ROWS] | [E, W_ROWS, K/128]
    const int* __restrict__ seg_off,       // [E+1] row offsets per expert
    const int* __restrict__ src_row,       // [R] source row per sorted row
    const int N,   // output width (I for gated, H for plain)
    const int K,
    const int E) {
  constexpr int NI = GATED ? 2 : 1;           // W images: gate, up
  constexpr int MT = BM / 16;                 // m tiles per wave
  constexpr int NV = QBITS == 4 ? 1 : 2;      // 16-B W vectors per lane-slab
  constexpr int VPR = QBITS == 4 ? 2 : 4;     // 16-B vectors per W row-slab
  constexpr float OFF = QBITS == 4 ? 8.f : 128.f;
  // register stages = slabs the global loads run ahead.  The 128-row tile's
  // accumulators leave room for one
  constexpr int NST = BM == 32 ? 2 : 1;

  // m-chunk slowest: the first chunks of all experts, which are the live
  // workgroups when segments are short, are dispatched together and spread
  // over the CUs.  With the chunks of one expert adjacent, the dead ones
  // exit at once and the next live workgroups land on the CUs they freed:
  // at MBLK >= 4 the down GEMM ran on a quarter of the device, at twice the
  // time (profiles/r09_moe_gemm_q.txt, section 2)
  const int e = blockIdx.y % E;
  const int mb = blockIdx.y / E;
  const int m_lo = seg_off[e] + mb * BM;
  const int m_hi = seg_off[e + 1];
  if (m_lo >= m_hi) return;
  const int M = min(BM, m_hi - m_lo);

  const int n0 = blockIdx.x * TQ_BN;
  const int nslabs = K / TQ_BK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row16 = lane & 15;
  const int kq = lane >> 4;

  __shared__ __hip_bfloat16 w_lds[2][NI][TQ_BN * TQ_BK];
  __shared__ __hip_bfloat16 x_lds[2][BM * TQ_BK];

  // ---- W staging: vector v of this lane is piece w_vec of tile row w_row;
  // image 0 holds rows n0.. of the expert (gate), image 1 rows N + n0.. (up)
  const long row_bytes = (long)K * QBITS / 8;
  const long w_rows = (long)NI * N;
  int w_row[NV], w_vec[NV];
  const unsigned char* w_src[NI][NV];
  const float* s_src[NI];
  float s8[NI][NV];      // int8 row scales, loaded once
  float st_s[NST][NI];   // int4 group scales, per stage
  u32x4_t st_w[NST][NI][NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int idx = v * 256 + tid;
    w_row[v] = idx / VPR;
    w_vec[v] = idx % VPR;
  }
#pragma unroll
  for (int im = 0; im < NI; ++im) {
    const long r0 = e * w_rows + (long)im * N + n0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      w_src[im][v] = wq + (r0 + w_row[v]) * row_bytes + w_vec[v] * 16;
      if (QBITS == 8) s8[im][v] = wscale[r0 + w_row[v]];
    }
    s_src[im] = wscale + (r0 + w_row[0]) * (K / TQ_GROUP);
  }

  auto load_w = [&](int st, int slab) {
#pragma unroll
    for (int im = 0; im < NI; ++im) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
        st_w[st][im][v] = *reinterpret_cast<const u32x4_t*>(
            w_src[im][v] + slab * (TQ_BK * QBITS / 8));
      if (QBITS == 4) st_s[st][im] = s_src[im][slab * TQ_BK / TQ_GROUP];
    }
  };

  auto write_w = [&](int st, int buf) {
#pragma unroll
    for (int im = 0; im < NI; ++im) {
      char* img = reinterpret_cast<char*>(w_lds[buf][im]);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float s = QBITS == 4 ? st_s[st][im] : s8[im][v];
        const float c = -OFF * s;
        if (QBITS == 4) {
#pragma unroll
          for (int d = 0; d < 4; ++d)
            *reinterpret_cast<u32x4_t*>(
                img + tq_swz(w_row[v], w_vec[v] * 4 + d)) =
                tq_dq4(st_w[st][im][v][d], s, c);
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<u32x4_t*>(
                img + tq_swz(w_row[v], w_vec[v] * 2 + h)) =
                tq_dq8(st_w[st][im][v][2 * h], st_w[st][im][v][2 * h + 1], s,
                       c);
        }
      }
    }
  };

  // ---- x staging: 8 lanes per 128-byte row, 32 rows per pass; the row
  // indices (through src_row for GATHER) are fixed for the whole k loop
  constexpr int XP = BM / 32;
  const int x_row = tid >> 3;
  const int x_k8 = tid & 7;
  const __hip_bfloat16* x_src[XP];
  bf16x8_t st_x[NST][XP];
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    const int r = m_lo + min(p * 32 + x_row, M - 1);
    x_src[p] = x + (long)(GATHER ? src_row[r] : r) * K + x_k8 * 8;
  }

  auto load_x = [&](int st, int slab) {
#pragma unroll
    for (int p = 0; p < XP; ++p)
      st_x[st][p] =
          *reinterpret_cast<const bf16x8_t*>(x_src[p] + slab * TQ_BK);
  };
  auto write_x = [&](int st, int buf) {
#pragma unroll
    for (int p = 0; p < XP; ++p)
      *reinterpret_cast<bf16x8_t*>(reinterpret_cast<char*>(x_lds[buf]) +
                                   tq_swz(p * 32 + x_row, x_k8)) = st_x[st][p];
  };

  f32x4_t acc[NI][2][MT];
#pragma unroll
  for (int im = 0; im < NI; ++im)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[im][j][i] = f32x4_t{};

  load_w(0, 0);
  load_x(0, 0);
  if (NST == 2 && nslabs > 1) {
    load_w(NST - 1, 1);
    load_x(NST - 1, 1);
  }

  for (int c0 = 0; c0 < nslabs; c0 += 2) {
#pragma unroll
    for (int buf = 0; buf < 2; ++buf) {  // unrolled: stages stay in registers
      const int c = c0 + buf;
      if (c >= nslabs) break;  // odd slab count, uniform over the workgroup
      constexpr int LAST = NST - 1;
      const int st = buf & LAST;
      // buffer buf was last read in slab c-2, which every wave finished
      // before it passed the barrier of slab c-1
      write_w(st, buf);
      write_x(st, buf);
      if (c + NST < nslabs) {  // lands under the next NST slabs' MFMAs
        load_w(st, c + NST);
        load_x(st, c + NST);
      }
      __syncthreads();

#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {  // two 32-deep k-steps per slab
        bf16x8_t a[NI][2], b[MT];
#pragma unroll
        for (int im = 0; im < NI; ++im)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            a[im][j] = *reinterpret_cast<const bf16x8_t*>(
                reinterpret_cast<const char*>(w_lds[buf][im]) +
                tq_swz(wave * 32 + j * 16 + row16, kk * 4 + kq));
#pragma unroll
        for (int i = 0; i < MT; ++i)
          b[i] = *reinterpret_cast<const bf16x8_t*>(
              reinterpret_cast<const char*>(x_lds[buf]) +
              tq_swz(i * 16 + row16, kk * 4 + kq));
#pragma unroll
        for (int im = 0; im < NI; ++im)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i)
              acc[im][j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[im][j], b[i], acc[im][j][i], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: C frag D[n_local = kq*4 + reg][m = row16] per (j, i):
  // four consecutive n of one row, f32 silu(g)*u, one rounding, 8-byte store
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long n = n0 + wave * 32 + j * 16 + kq * 4;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = i * 16 + row16;
      if (m >= M) continue;
      f32x4_t v = acc[0][j][i];
      if (GATED) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          v[r] = v[r] / (1.f + __expf(-v[r])) * acc[NI - 1][j][i][r];
      }
      u32x2_t o;
      o[0] = tq_pk_bf16(v[0], v[1]);
      o[1] = tq_pk_bf16(v[2], v[3]);
      *reinterpret_cast<u32x2_t*>(y + (long)(m_lo + m) * N + n) = o;
    }
  }
}

// x rows per workgroup: pure function of (R, E).  The 128-row tile once the
// mean segment is longer than the small tile.
int moe_gemm_q_block_m(int R, int E) { return R > 32 * E ? 128 : 32; }

template <int QBITS, int BM>
static void launch_mq(__hip_bfloat16* y, const __hip_bfloat16* x,
                      const unsigned char* wq, const float* ws,
                      const int* seg_off, const int* src_row, int E, int N,
                      int K, int R, bool gated, hipStream_t stream) {
  const int mblk = (R + BM - 1) / BM;
  const dim3 grid(N / TQ_BN, E * mblk);
#define MQ_LAUNCH(GATED, GATHER)                                             \
  hipLaunchKernelGGL((moe_gemm_q_kernel<QBITS, GATED, GATHER, BM>), grid,    \
                     dim3(256), 0, stream, y, x, wq, ws, seg_off, src_row,   \
                     N, K, E)
  if (src_row) {
    if (gated) MQ_LAUNCH(true, true);
    else MQ_LAUNCH(false, true);
  } else {
    if (gated) MQ_LAUNCH(true, false);
    else MQ_LAUNCH(false, false);
  }
#undef MQ_LAUNCH
}

// src_row == nullptr: x is already sorted by expert.  R counts the sorted
// rows (y's rows); E * ceil(R / moe_gemm_q_block_m(R, E)) must fit grid.y.
void launch_moe_gemm_q(__hip_bfloat16* y, const __hip_bfloat16* x,
                       const unsigned char* wq, const float* ws,
                       const int* seg_off, const int* src_row, int qbits,
                       int E, int N, int K, int R, bool gated,
                       hipStream_t stream) {
  const bool tall = moe_gemm_q_block_m(R, E) == 128;
  if (qbits == 8) {
    if (tall) launch_mq<8, 128>(y, x, wq, ws, seg_off, src_row, E, N, K, R, gated, stream);
    else launch_mq<8, 32>(y, x, wq, ws, seg_off, src_row, E, N, K, R, gated, stream);
  } else {
    if (tall) launch_mq<4, 128>(y, x, wq, ws, seg_off, src_row, E, N, K, R, gated, stream);
    else launch_mq<4, 32>(y, x, wq, ws, seg_off, src_row, E, N, K, R, gated, stream);
  }
}
