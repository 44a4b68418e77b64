// Weight-only-quantized tile GEMM for M > 64:
//   y[M,N] = x[M,K] @ dequant(Wq)[N,K]^T, x/y bf16, f32 accumulation on
//   v_mfma_f32_16x16x32_bf16.
// Storage is that of gemm_skinny_q.hip, unchanged: int8 wq [N][K] with
// scales [N]; int4 wq [N][K/2] offset-binary nibbles (even k low) with
// scales [N][K/128].
//
// Tile: BM(64|128) x 128(N) x 64(K) per 4-wave workgroup; wave w owns the
// 32 W rows [32w, 32w+32) against all BM x rows (BM/16 x 2 accumulator
// tiles).  The dequant cost of a slab is 128 x 64 conversions whatever BM
// is, so BM=128 halves the VALU work per MFMA; BM=64 is used while a
// 128-row tiling would leave CUs idle (tq_block_m, a pure shape function).
// LDS per workgroup: W 2 x 16 KB + x 2 x BM*128 B -> 48 KB (3 per CU) or
// 64 KB (2 per CU).
//
// W path: each lane fetches 16 packed bytes per vector (32 int4 / 16 int8
// weights) into registers one slab ahead, so the loads fly under the current
// slab's MFMAs; the int4 group scale rides along as one more independent
// load of that stage (a slab never straddles a 128-k group because the
// K-split keeps every workgroup's k range a multiple of 128).  At the top of
// the next iteration the registers are converted and written to LDS as bf16.
// x takes the same register route (16 B per lane, 8 lanes per row).  A
// global_load_lds x path was tried first: the compiler cannot tell the two
// x buffers apart and put s_waitcnt vmcnt(0) in front of the fragment reads,
// which also drained the W prefetch it was meant to overlap.
//
// Both LDS images are [rows][64] bf16 with the 16-byte slot of a row rotated
// by row>>1 (gemm_tile.hip's skew): the ds_read_b128 fragment reads of 16
// consecutive rows at one k8 slot hit distinct banks.
//
// Exact values: a weight byte b in offset-binary (int4 nibble: q+8; int8:
// q+128 after flipping the sign bit) is converted with v_cvt_f32_ubyte and
// one fma(b, s, -off*s).  off*s is exact (power-of-two multiple) and the fma
// rounds the exact product q*s once, so the f32 equals torch's q.float()*s;
// v_cvt_pk_bf16_f32 then rounds to nearest even as torch's .to(bf16) does.
// dequant_weight_kernel below uses the same routine and is checked
// bit-for-bit against ops.dequantize_weight's torch chain.
//
// Small grids get a K-split (tq_num_ksplit, pure shape function, no atomics)
// with f32 partials merged by gemm_skinny_merge_kernel.  x rows past M are
// read from row M-1 (in bounds) and their results are never written.

#include "quant_cvt.h"  // storage constants, LDS skew, exact conversions

// QBITS: 8 or 4.  BM: 64 or 128 x rows per workgroup.
template <int QBITS, int BM>
__global__ __launch_bounds__(256, BM == 64 ? 3 : 2) void gemm_tile_q_kernel(
    __hip_bfloat16* __restrict__ y,        // [M, N]        (KS == 1)
    float* __restrict__ part,              // [KS, M, N]    (KS > 1) or null
    const __hip_bfloat16* __restrict__ x,  // [M, K]
    const unsigned char* __restrict__ wq,  // int8: [N][K]; int4: [N][K/2]
    const float* __restrict__ wscale,      // int8: [N]; int4: [N][K/128]
    const int M, const int N, const int K) {
  constexpr int MT = BM / 16;                 // m tiles per wave
  constexpr int NV = QBITS == 4 ? 1 : 2;      // 16-B W vectors per lane-slab
  constexpr int VPR = QBITS == 4 ? 2 : 4;     // 16-B vectors per W row-slab
  constexpr float OFF = QBITS == 4 ? 8.f : 128.f;

  const int m0 = blockIdx.x * BM;  // m fastest: neighbours share the W tile
  const int n0 = blockIdx.y * TQ_BN;
  const int ks = blockIdx.z;
  const int KS = gridDim.z;
  const int k_per_wg = K / KS;
  const int k_lo = ks * k_per_wg;
  const int nslabs = k_per_wg / TQ_BK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row16 = lane & 15;
  const int kq = lane >> 4;

  __shared__ __hip_bfloat16 w_lds[2][TQ_BN * TQ_BK];
  __shared__ __hip_bfloat16 x_lds[2][BM * TQ_BK];

  // ---- W staging: vector v of this lane is piece w_vec of tile row w_row --
  const long row_bytes = (long)K * QBITS / 8;
  int w_row[NV], w_vec[NV];
  const unsigned char* w_src[NV];
  float st_s[NV];
  u32x4_t st_w[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int idx = v * 256 + tid;
    w_row[v] = idx / VPR;
    w_vec[v] = idx % VPR;
    w_src[v] = wq + (n0 + w_row[v]) * row_bytes + (long)k_lo * QBITS / 8 +
               w_vec[v] * 16;
    if (QBITS == 8) st_s[v] = wscale[n0 + w_row[v]];
  }
  const float* s_src =
      wscale + (long)(n0 + w_row[0]) * (K / TQ_GROUP) + k_lo / TQ_GROUP;

  auto load_w = [&](int slab) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      st_w[v] = *reinterpret_cast<const u32x4_t*>(
          w_src[v] + slab * (TQ_BK * QBITS / 8));
    if (QBITS == 4) st_s[0] = s_src[slab * TQ_BK / TQ_GROUP];
  };

  auto write_w = [&](int buf) {
    char* img = reinterpret_cast<char*>(w_lds[buf]);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float s = st_s[v];
      const float c = -OFF * s;
      if (QBITS == 4) {
#pragma unroll
        for (int d = 0; d < 4; ++d)
          *reinterpret_cast<u32x4_t*>(
              img + tq_swz(w_row[v], w_vec[v] * 4 + d)) =
              tq_dq4(st_w[v][d], s, c);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          *reinterpret_cast<u32x4_t*>(
              img + tq_swz(w_row[v], w_vec[v] * 2 + h)) =
              tq_dq8(st_w[v][2 * h], st_w[v][2 * h + 1], s, c);
      }
    }
  };

  // ---- x staging: 8 lanes per 128-byte row, 32 rows per pass --------------
  constexpr int XP = BM / 32;
  const int x_row = tid >> 3;
  const int x_k8 = tid & 7;
  const __hip_bfloat16* x_src[XP];
  bf16x8_t st_x[XP];
#pragma unroll
  for (int p = 0; p < XP; ++p)
    x_src[p] = x + (long)min(m0 + p * 32 + x_row, M - 1) * K + k_lo + x_k8 * 8;

  auto load_x = [&](int slab) {
#pragma unroll
    for (int p = 0; p < XP; ++p)
      st_x[p] = *reinterpret_cast<const bf16x8_t*>(x_src[p] + slab * TQ_BK);
  };
  auto write_x = [&](int buf) {
#pragma unroll
    for (int p = 0; p < XP; ++p)
      *reinterpret_cast<bf16x8_t*>(reinterpret_cast<char*>(x_lds[buf]) +
                                   tq_swz(p * 32 + x_row, x_k8)) = st_x[p];
  };

  f32x4_t acc[2][MT];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[j][i] = f32x4_t{};

  load_w(0);
  load_x(0);

  for (int c = 0; c < nslabs; ++c) {
    const int buf = c & 1;
    // buf was last read in slab c-2, which every wave finished before it
    // passed the barrier of slab c-1
    write_w(buf);
    write_x(buf);
    if (c + 1 < nslabs) {  // lands under this slab's MFMAs
      load_w(c + 1);
      load_x(c + 1);
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // two 32-deep k-steps per slab
      bf16x8_t a[2], b[MT];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        a[j] = *reinterpret_cast<const bf16x8_t*>(
            reinterpret_cast<const char*>(w_lds[buf]) +
            tq_swz(wave * 32 + j * 16 + row16, kk * 4 + kq));
#pragma unroll
      for (int i = 0; i < MT; ++i)
        b[i] = *reinterpret_cast<const bf16x8_t*>(
            reinterpret_cast<const char*>(x_lds[buf]) +
            tq_swz(i * 16 + row16, kk * 4 + kq));
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i)
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[j], b[i], acc[j][i], 0, 0, 0);
    }
  }

  // ---- epilogue: C frag D[n_local = kq*4 + reg][m = row16] per (j, i) -----
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long n = n0 + wave * 32 + j * 16 + kq * 4;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + i * 16 + row16;
      if (m >= M) continue;
      if (part == nullptr) {
        u32x2_t o;
        o[0] = tq_pk_bf16(acc[j][i][0], acc[j][i][1]);
        o[1] = tq_pk_bf16(acc[j][i][2], acc[j][i][3]);
        *reinterpret_cast<u32x2_t*>(y + (long)m * N + n) = o;
      } else {
        *reinterpret_cast<f32x4_t*>(part + ((long)ks * M + m) * N + n) =
            acc[j][i];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// One-pass dequant: wq, scales -> bf16 [N, K].  One 16-byte load per lane,
// 16-byte stores, values identical to the tile kernel's LDS image.
// ---------------------------------------------------------------------------

template <int QBITS>
__global__ __launch_bounds__(256) void dequant_weight_kernel(
    __hip_bfloat16* __restrict__ out,      // [N, K]
    const unsigned char* __restrict__ wq,
    const float* __restrict__ wscale,
    const long nvec,                       // N * K * QBITS / 128
    const int K) {
  constexpr int EPV = 128 / QBITS;  // weights per 16-byte vector
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const long e0 = v * EPV;  // K % 128 == 0: a vector stays in one row/group
  const long row = e0 / K;
  const int k = (int)(e0 - row * K);
  const u32x4_t u = *reinterpret_cast<const u32x4_t*>(wq + v * 16);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(out + e0);
  if (QBITS == 4) {
    const float s = wscale[row * (K / TQ_GROUP) + k / TQ_GROUP];
    const float c = -8.f * s;
#pragma unroll
    for (int d = 0; d < 4; ++d) dst[d] = tq_dq4(u[d], s, c);
  } else {
    const float s = wscale[row];
    const float c = -128.f * s;
    dst[0] = tq_dq8(u[0], u[1], s, c);
    dst[1] = tq_dq8(u[2], u[3], s, c);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

__global__ void gemm_skinny_merge_kernel(__hip_bfloat16*, const float*, int,
                                         int, int);  // gemm_skinny.hip

// 128-row tiles once they alone put a workgroup on every CU (256), else 64.
static int tq_block_m(int M, int N) {
  return ((M + 127) / 128) * (N / TQ_BN) >= 256 ? 128 : 64;
}

// KS: pure function of the shape (hipGraph-stable).  Doubles while the grid
// stays within two workgroups per CU and each workgroup keeps a k range that
// is a multiple of the int4 scale group and at least 512 deep.
int gemm_tile_q_num_ksplit(int M, int N, int K) {
  const int bm = tq_block_m(M, N);
  const int wgs = ((M + bm - 1) / bm) * (N / TQ_BN);
  int ks = 1;
  while (ks < 8 && wgs * ks * 2 <= 512 && (K / (ks * 2)) % TQ_GROUP == 0 &&
         K / (ks * 2) >= 512)
    ks *= 2;
  return ks;
}

template <int QBITS, int BM>
static void launch_tq(__hip_bfloat16* y, float* part, const __hip_bfloat16* x,
                      const unsigned char* wq, const float* ws, int M, int N,
                      int K, int KS, hipStream_t stream) {
  hipLaunchKernelGGL((gemm_tile_q_kernel<QBITS, BM>),
                     dim3((M + BM - 1) / BM, N / TQ_BN, KS), dim3(256), 0,
                     stream, y, part, x, wq, ws, M, N, K);
}

// part: [KS, M, N] f32 workspace when KS = gemm_tile_q_num_ksplit(...) > 1
void launch_gemm_tile_q(__hip_bfloat16* y, float* part,
                        const __hip_bfloat16* x, const unsigned char* wq,
                        const float* ws, int qbits, int M, int N, int K,
                        int KS, hipStream_t stream) {
  float* p = KS > 1 ? part : nullptr;
  const bool tall = tq_block_m(M, N) == 128;
  if (qbits == 8) {
    if (tall) launch_tq<8, 128>(y, p, x, wq, ws, M, N, K, KS, stream);
    else launch_tq<8, 64>(y, p, x, wq, ws, M, N, K, KS, stream);
  } else {
    if (tall) launch_tq<4, 128>(y, p, x, wq, ws, M, N, K, KS, stream);
    else launch_tq<4, 64>(y, p, x, wq, ws, M, N, K, KS, stream);
  }
  if (KS > 1) {
    const long total = (long)M * N;
    hipLaunchKernelGGL(gemm_skinny_merge_kernel, dim3((total + 255) / 256),
                       dim3(256), 0, stream, y, part, M, N, KS);
  }
}

void launch_dequant_weight(__hip_bfloat16* out, const unsigned char* wq,
                           const float* ws, int qbits, int N, int K,
                           hipStream_t stream) {
  const long nvec = (long)N * K * qbits / 128;
  const dim3 grid((unsigned)((nvec + 255) / 256));
  if (qbits == 8)
    hipLaunchKernelGGL(dequant_weight_kernel<8>, grid, dim3(256), 0, stream,
                       out, wq, ws, nvec, K);
  else
    hipLaunchKernelGGL(dequant_weight_kernel<4>, grid, dim3(256), 0, stream,
                       out, wq, ws, nvec, K);
}
