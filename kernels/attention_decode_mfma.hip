// MFMA paged decode attention — replaces the VALU decode
// kernel for bf16 head_dim 64/128, GQA group <= 8.
//
// The VALU kernel spent its time in per-slot cross-lane reduction chains
// (rocprofv3 r1: 155 us/call vs a ~17 us HBM roofline at batch 64, ctx 512).
// Here Q·K^T runs on v_mfma_f32_32x32x16_bf16 tiles with the swapped-operand
// trick from the prefill kernel (S^T = K·Q^T, so softmax stats are per-lane
// column with ONE shfl per 32-slot tile), and P is repacked with
// v_cvt_pk_bf16_f32 + v_permlane32_swap into the P·V A-operand.
//
// Memory side (the kernel is a KV stream: 2 bytes per K and V element, once):
//   * K and V rows are both fetched 16 lanes across one contiguous row, so
//     every load instruction covers whole cache lines, and both are staged
//     through a per-wave LDS image (no barriers: a wave only ever touches its
//     own image, and LDS operations of one wave execute in order).
//   * The loop is software-pipelined: tile t+1's global loads are issued
//     right after tile t's registers have been written to LDS and stay in
//     flight under tile t's QK^T, softmax and PV.
//   * K image: [32][HEAD_DIM] bf16 with byte ^= ((row & m) << 4) so the
//     ds_read_b128 A-fragment reads (one row per lane) are conflict-free.
//   * V image: HEAD_DIM/16 subtiles [32 kv][16 d] row-major, 1152 B apart,
//     read as B fragments with the hardware transpose ds_read_b64_tr_b16
//     (same layout as attention_prefill_mfma_v2.hip).
//   * The accumulator rescale (16 cross-lane shuffles + 16*DT multiplies) is
//     skipped for tiles in which no column's running max moved; the factor
//     is exactly 1.0 there, so results are unchanged.
//
// Flash-decoding split: grid (nseq, kvh, npart); the context is cut into
// npart contiguous tile ranges and each workgroup's 4 waves take tiles
// round-robin inside their range.  With npart > 1 every wave writes an
// independent partial (m, l, acc_f32) and a small merge kernel reduces the
// npart*4 partials per (seq, head).  With npart == 1 (every batch that fills
// the device on its own) the four waves merge through LDS with the same
// arithmetic and write bf16 `out` directly: no partials traffic, no second
// launch.  npart is a pure function of tensor shapes, so the launch is
// hipGraph-stable while the in-kernel split adapts to the runtime seq_len.

#include "common.h"
#include <float.h>

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_d;
typedef __attribute__((address_space(3))) bf16x4_d* lds_tr_ptr_d;

// 8 consecutive KV elements as bf16: direct for bf16 caches, hardware
// cvt_pk_f32_fp8 for e4m3 caches (fp8 KV halves the decode HBM stream)
template <typename CT>
DEVINLINE bf16x8_t load_kv8(const CT* p);
template <>
DEVINLINE bf16x8_t load_kv8<__hip_bfloat16>(const __hip_bfloat16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}
template <>
DEVINLINE bf16x8_t load_kv8<unsigned char>(const unsigned char* p) {
  return __builtin_bit_cast(
      bf16x8_t, fp8x8_to_bf16x8(*reinterpret_cast<const u32x2_vec_t*>(p)));
}

#define KVT 32     // kv slots per mfma tile
#define NWAVES 4   // waves per workgroup
#define MAX_GROUP 8
#define VSUB_BYTES 1152  // one [32 kv][16 d] V subtile + 128 B bank pad

template <int HEAD_DIM, typename CT, bool DIRECT>
__global__ __launch_bounds__(256, 2) void paged_decode_mfma_kernel(
    __hip_bfloat16* __restrict__ out,  // [nseq, nheads, HD] (DIRECT only)
    float* __restrict__ part_acc,   // [nseq, nheads, P, HEAD_DIM] f32
    float* __restrict__ part_ml,    // [nseq, nheads, P, 2] f32 (m, l)
    const __hip_bfloat16* __restrict__ q,        // [nseq, nheads, HD]
    const CT* __restrict__ k_cache,  // [nb, bs, kvh, HD] bf16 | e4m3
    const CT* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [nseq, max_blocks]
    const int* __restrict__ seq_lens,      // [nseq]
    const float scale,
    const int nheads,
    const int kvh,
    const int group,       // nheads / kvh, <= 8
    const int block_size,
    const int max_blocks) {
  constexpr int KCH = HEAD_DIM / 16;  // k-chunks for the QK^T mfma
  constexpr int DT = HEAD_DIM / 32;   // 32-col output tiles
  constexpr int ROW_BYTES = HEAD_DIM * 2;
  constexpr int K_SWZ = ROW_BYTES / 16 - 1;  // row bits folded into the 16-B slot
  constexpr int K_BYTES = KVT * ROW_BYTES;
  constexpr int V_BYTES = (HEAD_DIM / 16) * VSUB_BYTES;
  constexpr int WAVE_LDS = K_BYTES + V_BYTES;
  static_assert(NWAVES * WAVE_LDS >=
                    NWAVES * MAX_GROUP * (HEAD_DIM + 2) * (int)sizeof(float),
                "the wave-merge scratch aliases the staging images");

  const int seq = blockIdx.x;
  const int kv_head = blockIdx.y;
  const int part = blockIdx.z;
  const int npart = gridDim.z;
  const int seq_len = seq_lens[seq];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;   // kv row of the A frag AND q col of the B frag
  const int half = lane >> 5;

  // this partition's tile range; waves stride by NWAVES inside it
  const int tiles_total = (seq_len + KVT - 1) / KVT;
  const int tpp = (tiles_total + npart - 1) / npart;
  const int tile_lo = part * tpp;
  const int tile_hi = min(tile_lo + tpp, tiles_total);

  const int head0 = kv_head * group;
  const int* btable = block_tables + (long)seq * max_blocks;
  const long kv_row_stride = (long)kvh * HEAD_DIM;

  // per-wave K and V staging images
  __shared__ __attribute__((aligned(16))) char lds_all[NWAVES * WAVE_LDS];
  char* k_lds = lds_all + wave * WAVE_LDS;
  char* v_lds = k_lds + K_BYTES;

  // ---- Q as B fragments: lane holds Q[q=col][ks*16 + half*8 + j] ---------
  bf16x8_t qb[KCH];
  if (col < group) {
    const __hip_bfloat16* q_row = q + ((long)seq * nheads + head0 + col) * HEAD_DIM;
#pragma unroll
    for (int ks = 0; ks < KCH; ++ks)
      qb[ks] = *reinterpret_cast<const bf16x8_t*>(q_row + ks * 16 + half * 8);
  } else {
#pragma unroll
    for (int ks = 0; ks < KCH; ++ks) qb[ks] = bf16x8_t{};
  }

  float m_state = -FLT_MAX;  // per q col (duplicated on lane and lane^32)
  float l_state = 0.f;
  f32x16_t acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = f32x16_t{};

  // staging map, same for K and V: LPR lanes across one row, 64/LPR rows per
  // pass.  Slots at or past seq_len are never dereferenced (neither the block
  // table entry nor the cache row) and stage zeros.
  constexpr int LPR = HEAD_DIM / 8;        // lanes per row
  constexpr int ROWS_PER_PASS = 64 / LPR;  // rows per pass per wave
  constexpr int NPASS = KVT / ROWS_PER_PASS;
  const int st_row = lane / LPR;
  const int st_d8 = (lane % LPR) * 8;
  bf16x8_t st_k[NPASS], st_v[NPASS];

  auto issue_loads = [&](int t) {
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int pos = t * KVT + pass * ROWS_PER_PASS + st_row;
      st_k[pass] = bf16x8_t{};
      st_v[pass] = bf16x8_t{};
      if (pos < seq_len) {
        const int block = btable[pos / block_size];
        const long row = ((long)block * block_size + pos % block_size) *
                             kv_row_stride +
                         (long)kv_head * HEAD_DIM + st_d8;
        st_k[pass] = load_kv8<CT>(k_cache + row);
        st_v[pass] = load_kv8<CT>(v_cache + row);
      }
    }
  };

  int t = tile_lo + wave;
  if (t < tile_hi) issue_loads(t);

  for (; t < tile_hi; t += NWAVES) {
    const int kv_base = t * KVT;

    // ---- tile t: registers -> LDS images ---------------------------------
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int s = pass * ROWS_PER_PASS + st_row;
      *reinterpret_cast<bf16x8_t*>(
          k_lds + s * ROW_BYTES + ((st_d8 * 2) ^ ((s & K_SWZ) << 4))) = st_k[pass];
    }
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int s = pass * ROWS_PER_PASS + st_row;
      *reinterpret_cast<bf16x8_t*>(
          v_lds + (st_d8 >> 4) * VSUB_BYTES + s * 32 + (st_d8 & 15) * 2) = st_v[pass];
    }

    // ---- tile t+NWAVES: loads go out now, land under this tile's math ----
    if (t + NWAVES < tile_hi) issue_loads(t + NWAVES);

    // ---- S^T = K · Q^T ---------------------------------------------------
    f32x16_t acc_s{};
#pragma unroll
    for (int ks = 0; ks < KCH; ++ks) {
      const bf16x8_t ka = *reinterpret_cast<const bf16x8_t*>(
          k_lds + col * ROW_BYTES + ((ks * 32 + half * 16) ^ ((col & K_SWZ) << 4)));
      acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qb[ks], acc_s, 0, 0, 0);
    }

    // ---- online softmax (stats per q col = this lane's col) --------------
    float s_val[16];
    float local_max = -FLT_MAX;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv_pos = kv_base + (r & 3) + 8 * (r >> 2) + 4 * half;
      float sv = acc_s[r] * scale;
      if (kv_pos >= seq_len) sv = -FLT_MAX;
      s_val[r] = sv;
      local_max = fmaxf(local_max, sv);
    }
    const float tile_max = fmaxf(local_max, __shfl_xor(local_max, 32, 64));
    const float m_new = fmaxf(m_state, tile_max);
    const bool max_moved = m_new > m_state;
    const float rescale = __expf(m_state - m_new);
    m_state = m_new;

    float p[16];
    float local_sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = s_val[r] == -FLT_MAX ? 0.f : __expf(s_val[r] - m_new);
      local_sum += p[r];
    }
    l_state = l_state * rescale + local_sum + __shfl_xor(local_sum, 32, 64);

    // rescale factors redistributed to the PV accumulator's q rows; when no
    // column's max moved every factor is exactly 1.0 and the pass is skipped
    if (__any(max_moved)) {
      float f_reg[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = (r & 3) + 8 * (r >> 2) + 4 * half;
        f_reg[r] = __shfl(rescale, qrow, 64);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[dt][r] *= f_reg[r];
      }
    }

    // ---- pack P to bf16 A-fragments (cvt_pk + permlane32_swap) -----------
    unsigned int pk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2"
                   : "=v"(pk[i]) : "v"(p[2 * i]), "v"(p[2 * i + 1]));
    }
    bf16x8_t pa[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      unsigned x0 = pk[4 * c + 0], x1 = pk[4 * c + 1];
      unsigned y0 = pk[4 * c + 2], y1 = pk[4 * c + 3];
      {
        auto r0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
        x0 = r0[0]; y0 = r0[1];
        auto r1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
        x1 = r1[0]; y1 = r1[1];
      }
      union { unsigned u[4]; bf16x8_t v; } u;
      u.u[0] = x0; u.u[1] = x1; u.u[2] = y0; u.u[3] = y1;
      pa[c] = u.v;
    }

    // ---- PV: out[q][d] += P[q][kv] V[kv][d] ------------------------------
    // B fragment: lane needs V[c*16 + half*8 + j][dt*32 + col], j = 0..7.
    // Each 16-lane quarter transposes a [4 kv][16 d] window per read.
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const char* sub = v_lds + (dt * 2 + (col >> 4)) * VSUB_BYTES + (lane & 15) * 8;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const char* w = sub + (c * 16 + half * 8) * 32;
        union { bf16x4_d h[2]; bf16x8_t v; } b;
        b.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr_d)w);
        b.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr_d)(w + 128));
        acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[c], b.v, acc_o[dt], 0, 0, 0);
      }
    }
  }

  if constexpr (DIRECT) {
    // ---- npart == 1: merge the four waves through LDS, write bf16 out ----
    // Same arithmetic, in the same order, as decode_merge_kernel over P = 4.
    float* mg_acc = reinterpret_cast<float*>(lds_all);  // [NWAVES][8][HD]
    float* mg_ml = mg_acc + NWAVES * MAX_GROUP * HEAD_DIM;  // [NWAVES][8][2]
    __syncthreads();  // every wave is done with its staging images
    if (lane < group) {
      mg_ml[(wave * MAX_GROUP + lane) * 2 + 0] = m_state;
      mg_ml[(wave * MAX_GROUP + lane) * 2 + 1] = l_state;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (qrow >= group) continue;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        mg_acc[(wave * MAX_GROUP + qrow) * HEAD_DIM + dt * 32 + col] = acc_o[dt][r];
    }
    __syncthreads();
    for (int e = tid; e < group * HEAD_DIM; e += NWAVES * 64) {
      const int h = e / HEAD_DIM;
      const int d = e % HEAD_DIM;
      float M = -FLT_MAX;
#pragma unroll
      for (int w = 0; w < NWAVES; ++w)
        M = fmaxf(M, mg_ml[(w * MAX_GROUP + h) * 2]);
      float L = 0.f, A = 0.f;
#pragma unroll
      for (int w = 0; w < NWAVES; ++w) {
        const float f = __expf(mg_ml[(w * MAX_GROUP + h) * 2] - M);
        // explicit fma: the merge kernel's loop compiles to fused ops, and
        // both paths must round alike
        L = __builtin_fmaf(f, mg_ml[(w * MAX_GROUP + h) * 2 + 1], L);
        A = __builtin_fmaf(f, mg_acc[(w * MAX_GROUP + h) * HEAD_DIM + d], A);
      }
      const float inv = L > 0.f ? 1.f / L : 0.f;
      out[((long)seq * nheads + head0 + h) * HEAD_DIM + d] = __float2bfloat16(A * inv);
    }
  } else {
    // ---- per-wave partial store: (m, l) per q col + f32 accumulator ------
    const int P = npart * NWAVES;
    const int pw = part * NWAVES + wave;
    if (lane < group) {
      float* ml = part_ml + (((long)seq * nheads + head0 + lane) * P + pw) * 2;
      ml[0] = m_state;
      ml[1] = l_state;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (qrow >= group) continue;
      float* acc_row =
          part_acc + (((long)seq * nheads + head0 + qrow) * P + pw) * HEAD_DIM;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc_row[dt * 32 + col] = acc_o[dt][r];
    }
  }
}

// Reduce the P partials of each (seq, head) row: out = sum_p f_p acc_p / sum_p f_p l_p
template <int HEAD_DIM>
__global__ void decode_merge_kernel(
    __hip_bfloat16* __restrict__ out,      // [nseq, nheads, HD]
    const float* __restrict__ part_acc,    // [nseq, nheads, P, HD]
    const float* __restrict__ part_ml,     // [nseq, nheads, P, 2]
    const int nheads,
    const int P) {
  const int seq = blockIdx.x;
  const int head = blockIdx.y;
  const int d = threadIdx.x;
  const long row = (long)seq * nheads + head;
  const float* ml = part_ml + row * P * 2;
  const float* acc = part_acc + row * P * HEAD_DIM + d;

  float M = -FLT_MAX;
  for (int p = 0; p < P; ++p) M = fmaxf(M, ml[2 * p]);
  float L = 0.f, A = 0.f;
  for (int p = 0; p < P; ++p) {
    const float f = __expf(ml[2 * p] - M);
    L += f * ml[2 * p + 1];
    A += f * acc[(long)p * HEAD_DIM];
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  out[row * HEAD_DIM + d] = __float2bfloat16(A * inv);
}

int decode_mfma_num_partitions(int nseq, int kvh, int max_context) {
  // pure function of shapes (hipGraph-stable): fill >=512 workgroups, but
  // keep >=2 tiles per partition at the allocated max context
  int npart = 512 / (nseq * kvh > 0 ? nseq * kvh : 1);
  if (npart < 1) npart = 1;
  if (npart > 32) npart = 32;
  const int max_tiles = (max_context + KVT - 1) / KVT;
  const int cap = max_tiles / 2 > 0 ? max_tiles / 2 : 1;
  if (npart > cap) npart = cap;
  return npart;
}

template <int HEAD_DIM, typename CT>
static void launch_decode_hd(__hip_bfloat16* out, float* part_acc,
                             float* part_ml, const __hip_bfloat16* q,
                             const CT* kc, const CT* vc, const int* bt,
                             const int* sl, float scale, int nseq, int nheads,
                             int kvh, int block_size, int max_blocks,
                             int npart, hipStream_t stream) {
  const int group = nheads / kvh;
  dim3 grid(nseq, kvh, npart);
  dim3 block(NWAVES * 64);
  if (npart == 1) {
    // part_acc / part_ml are not touched on this path
    hipLaunchKernelGGL((paged_decode_mfma_kernel<HEAD_DIM, CT, true>), grid,
                       block, 0, stream, out, part_acc, part_ml, q, kc, vc, bt,
                       sl, scale, nheads, kvh, group, block_size, max_blocks);
    return;
  }
  hipLaunchKernelGGL((paged_decode_mfma_kernel<HEAD_DIM, CT, false>), grid,
                     block, 0, stream, out, part_acc, part_ml, q, kc, vc, bt,
                     sl, scale, nheads, kvh, group, block_size, max_blocks);
  hipLaunchKernelGGL(decode_merge_kernel<HEAD_DIM>, dim3(nseq, nheads),
                     dim3(HEAD_DIM), 0, stream, out, part_acc, part_ml, nheads,
                     npart * NWAVES);
}

template <typename CT>
static void launch_decode_ct(__hip_bfloat16* out, float* part_acc,
                             float* part_ml, const __hip_bfloat16* q,
                             const CT* kc, const CT* vc, const int* bt,
                             const int* sl, float scale, int nseq, int nheads,
                             int kvh, int head_dim, int block_size,
                             int max_blocks, int npart, hipStream_t stream) {
  switch (head_dim) {
    case 64:
      launch_decode_hd<64, CT>(out, part_acc, part_ml, q, kc, vc, bt, sl, scale,
                               nseq, nheads, kvh, block_size, max_blocks, npart,
                               stream);
      break;
    case 128:
      launch_decode_hd<128, CT>(out, part_acc, part_ml, q, kc, vc, bt, sl,
                                scale, nseq, nheads, kvh, block_size,
                                max_blocks, npart, stream);
      break;
    default:
      abort();
  }
}

void launch_paged_decode_mfma(__hip_bfloat16* out, float* part_acc,
                              float* part_ml, const __hip_bfloat16* q,
                              const __hip_bfloat16* kc, const __hip_bfloat16* vc,
                              const int* bt, const int* sl, float scale,
                              int nseq, int nheads, int kvh, int head_dim,
                              int block_size, int max_blocks, int npart,
                              hipStream_t stream) {
  launch_decode_ct<__hip_bfloat16>(out, part_acc, part_ml, q, kc, vc, bt, sl,
                                   scale, nseq, nheads, kvh, head_dim,
                                   block_size, max_blocks, npart, stream);
}

void launch_paged_decode_mfma_fp8(
    __hip_bfloat16* out, float* part_acc, float* part_ml,
    const __hip_bfloat16* q, const unsigned char* kc, const unsigned char* vc,
    const int* bt, const int* sl, float scale, int nseq, int nheads, int kvh,
    int head_dim, int block_size, int max_blocks, int npart,
    hipStream_t stream) {
  launch_decode_ct<unsigned char>(out, part_acc, part_ml, q, kc, vc, bt, sl,
                                  scale, nseq, nheads, kvh, head_dim,
                                  block_size, max_blocks, npart, stream);
}
