// MFMA paged attention for short query chunks over a long cached context
// (speculative verify, prefix-cache hits): q_len new tokens per sequence,
// q_len * group <= 32 (head_dim 128) or 64 (head_dim 64).
//
// The prefill kernels put one query head per workgroup, so a GQA group of g
// streams the sequence's KV g times and a 256-row q tile carries q_len real
// rows.  Here the whole chunk of one KV head is ONE pass over the KV stream,
// as in attention_decode_mfma.hip: S^T = K·Q^T on v_mfma_f32_32x32x16_bf16
// with Q as the 32-column B operand.  Decode fills `group` of those columns;
// this kernel fills q_len * group of them:
//
//   column c of column block b  <->  query token j = (b*32 + c) / group,
//                                    head        h = (b*32 + c) % group
//
// and every column carries its own causal limit
//   kv_pos < seq_len - q_len + j + 1.
// Columns past q_len * group hold zero Q, a limit of 0 (always masked) and
// are never written out.  With q_len == 1 the map, the limit and every
// floating-point operation are those of the decode kernel, so verify rows and
// decode rows agree bit for bit (tests/test_multiq_attention_gpu.py).
//
// NQB = 1 serves q_len * group <= 32.  NQB = 2 (head_dim 64) serves <= 64
// with a second column block: the Q fragments of both blocks sit in an LDS
// image in fragment order ([block][k-chunk][lane] x 16 B, conflict-free
// ds_read_b128) to leave the registers to two blocks of PV accumulators.  The
// two blocks run back to back on the same staged tile: the K A-fragments and
// V B-fragments are re-read from LDS (LDS traffic is a small multiple of the
// HBM stream), global memory is read once.  At head_dim 128 two blocks need
// 128 accumulator registers on top of the 32 staging registers; with the 256
// registers that two workgroups per CU leave a wave the compiler spills to
// scratch, so that instantiation is not built and head_dim 128 stops at
// q_len * group <= 32.
//
// Memory side, work split and merge are the decode kernel's: K and V fetched
// 16 lanes per contiguous row, per-wave LDS images (K XOR-swizzled for
// ds_read_b128, V in [32 kv][16 d] subtiles read with ds_read_b64_tr_b16), the
// loads of tile t+4 in flight under tile t's math, rescale skipped when no
// column's max moved, grid (seq, kv_head, npart) with
// decode_mfma_num_partitions, in-kernel LDS merge of the four waves when
// npart == 1 and f32 partials plus a merge kernel otherwise.  Tiles at or past
// seq_len are not loaded and their block-table entries are not read.

#include "common.h"
#include <float.h>

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_d;
typedef __attribute__((address_space(3))) bf16x4_d* lds_tr_ptr_d;

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

constexpr int KVT = 32;     // kv slots per mfma tile
constexpr int NWAVES = 4;   // waves per workgroup
constexpr int QCOLS = 32;   // q columns per column block (the mfma N)
constexpr int VSUB_BYTES = 1152;  // one [32 kv][16 d] V subtile + 128 B bank pad

// Query rows of one sequence, clipped to the q tensor: a start or end outside
// [0, total_tokens] can only shorten the chunk, never move an access outside
// q / out.
DEVINLINE int chunk_len(int q0, int q1, int total_tokens) {
  if (q0 < 0) return 0;
  return min(q1, total_tokens) - q0;
}

template <int HEAD_DIM, typename CT, int NQB, bool DIRECT>
__global__ __launch_bounds__(256, 2) void paged_multiq_mfma_kernel(
    __hip_bfloat16* __restrict__ out,  // [T, nheads, HD] (DIRECT only)
    float* __restrict__ part_acc,   // [T, nheads, P, HEAD_DIM] f32
    float* __restrict__ part_ml,    // [T, nheads, P, 2] f32 (m, l)
    const __hip_bfloat16* __restrict__ q,        // [T, nheads, HD]
    const CT* __restrict__ k_cache,  // [nb, bs, kvh, HD] bf16 | e4m3
    const CT* __restrict__ v_cache,
    const int* __restrict__ block_tables,     // [nseq, max_blocks]
    const int* __restrict__ query_start_loc,  // [nseq + 1]
    const int* __restrict__ seq_lens,         // [nseq]
    const float scale,
    const int nheads,
    const int kvh,
    const int group,       // nheads / kvh, <= 8
    const int block_size,
    const int max_blocks,
    const int total_tokens) {
  constexpr int KCH = HEAD_DIM / 16;  // k-chunks for the QK^T mfma
  constexpr int DT = HEAD_DIM / 32;   // 32-col output tiles
  constexpr int ROW_BYTES = HEAD_DIM * 2;
  constexpr int K_SWZ = ROW_BYTES / 16 - 1;  // row bits folded into the 16-B slot
  constexpr int K_BYTES = KVT * ROW_BYTES;
  constexpr int Q_LDS = NQB == 2 ? NQB * KCH * 64 * 16 : 0;  // Q fragments
  constexpr int V_BYTES = (HEAD_DIM / 16) * VSUB_BYTES;
  constexpr int WAVE_LDS = K_BYTES + V_BYTES;
  constexpr int LDS_BYTES = NWAVES * WAVE_LDS + Q_LDS;
  static_assert(NQB == 1 || (NQB == 2 && HEAD_DIM == 64),
                "two column blocks: head_dim 64 only (see the file comment)");
  static_assert(LDS_BYTES >=
                    NWAVES * QCOLS * (HEAD_DIM + 2) * (int)sizeof(float),
                "the wave-merge scratch aliases the staging and Q images");
  static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

  const int seq = blockIdx.x;
  const int kv_head = blockIdx.y;
  const int part = blockIdx.z;
  const int npart = gridDim.z;
  const int seq_len = seq_lens[seq];
  const int q0 = query_start_loc[seq];
  const int q_len = chunk_len(q0, query_start_loc[seq + 1], total_tokens);
  if (q_len <= 0) return;  // empty chunk: nothing to write (workgroup-uniform)
  const int ncols = min(q_len * group, NQB * QCOLS);

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

  // per-wave K and V staging images, then the Q image (NQB == 2)
  __shared__ __attribute__((aligned(16))) char lds_all[LDS_BYTES];
  char* k_lds = lds_all + wave * WAVE_LDS;
  char* v_lds = k_lds + K_BYTES;
  char* q_lds = lds_all + NWAVES * WAVE_LDS;

  // ---- column map and causal limits --------------------------------------
  // lane's column in block b: token j, head h; limit 0 masks an unused column
  int limit[NQB];
  long q_off[NQB];  // element offset of the column's Q row, -1 = unused
#pragma unroll
  for (int b = 0; b < NQB; ++b) {
    const int c = b * QCOLS + col;
    const int j = c / group;
    const int h = c - j * group;
    const bool used = c < ncols;
    limit[b] = used ? seq_len - q_len + j + 1 : 0;
    q_off[b] = used ? ((long)(q0 + j) * nheads + head0 + h) * HEAD_DIM : -1;
  }

  // ---- Q as B fragments: lane holds Q[q=col][ks*16 + half*8 + j] ---------
  // NQB == 1: in registers.  NQB == 2: in the LDS image, [block][ks][lane].
  bf16x8_t qb[KCH];
  const bool blk1 = NQB == 2 && ncols > QCOLS;  // workgroup-uniform
  if constexpr (NQB == 1) {
    if (q_off[0] >= 0) {
      const __hip_bfloat16* q_row = q + q_off[0];
#pragma unroll
      for (int ks = 0; ks < KCH; ++ks)
        qb[ks] = *reinterpret_cast<const bf16x8_t*>(q_row + ks * 16 + half * 8);
    } else {
#pragma unroll
      for (int ks = 0; ks < KCH; ++ks) qb[ks] = bf16x8_t{};
    }
  } else {
    // wave w stages k-chunks w, w+4, ... of both blocks for the workgroup
#pragma unroll
    for (int b = 0; b < NQB; ++b) {
#pragma unroll
      for (int ks = wave; ks < KCH; ks += NWAVES) {
        bf16x8_t f{};
        if (q_off[b] >= 0)
          f = *reinterpret_cast<const bf16x8_t*>(q + q_off[b] + ks * 16 + half * 8);
        *reinterpret_cast<bf16x8_t*>(q_lds + ((b * KCH + ks) * 64 + lane) * 16) = f;
      }
    }
    __syncthreads();
  }

  float m_state[NQB], l_state[NQB];  // per q col (duplicated on lane, lane^32)
  f32x16_t acc_o[NQB][DT];
#pragma unroll
  for (int b = 0; b < NQB; ++b) {
    m_state[b] = -FLT_MAX;
    l_state[b] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_o[b][dt] = f32x16_t{};
  }

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

#pragma unroll
    for (int b = 0; b < NQB; ++b) {
      if (b == 1 && !blk1) continue;

      // ---- S^T = K · Q^T -------------------------------------------------
      f32x16_t acc_s{};
#pragma unroll
      for (int ks = 0; ks < KCH; ++ks) {
        const bf16x8_t ka = *reinterpret_cast<const bf16x8_t*>(
            k_lds + col * ROW_BYTES + ((ks * 32 + half * 16) ^ ((col & K_SWZ) << 4)));
        bf16x8_t qf;
        if constexpr (NQB == 1)
          qf = qb[ks];
        else
          qf = *reinterpret_cast<const bf16x8_t*>(
              q_lds + ((b * KCH + ks) * 64 + lane) * 16);
        acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf, acc_s, 0, 0, 0);
      }

      // ---- online softmax (stats per q col = this lane's col) ------------
      // a column whose whole tile is masked gets tile_max = -FLT_MAX, so
      // m_new == m_state, rescale == 1 and every p == 0: state unchanged
      float s_val[16];
      float local_max = -FLT_MAX;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_pos = kv_base + (r & 3) + 8 * (r >> 2) + 4 * half;
        float sv = acc_s[r] * scale;
        if (kv_pos >= limit[b]) sv = -FLT_MAX;
        s_val[r] = sv;
        local_max = fmaxf(local_max, sv);
      }
      const float tile_max = fmaxf(local_max, __shfl_xor(local_max, 32, 64));
      const float m_new = fmaxf(m_state[b], tile_max);
      const bool max_moved = m_new > m_state[b];
      const float rescale = __expf(m_state[b] - m_new);
      m_state[b] = m_new;

      float p[16];
      float local_sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = s_val[r] == -FLT_MAX ? 0.f : __expf(s_val[r] - m_new);
        local_sum += p[r];
      }
      l_state[b] = l_state[b] * rescale + local_sum + __shfl_xor(local_sum, 32, 64);

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
          for (int r = 0; r < 16; ++r) acc_o[b][dt][r] *= f_reg[r];
        }
      }

      // ---- pack P to bf16 A-fragments (cvt_pk + permlane32_swap) ---------
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

      // ---- PV: out[q][d] += P[q][kv] V[kv][d] ----------------------------
      // B fragment: lane needs V[c*16 + half*8 + j][dt*32 + col], j = 0..7.
      // Each 16-lane quarter transposes a [4 kv][16 d] window per read.
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const char* sub = v_lds + (dt * 2 + (col >> 4)) * VSUB_BYTES + (lane & 15) * 8;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const char* w = sub + (c * 16 + half * 8) * 32;
          union { bf16x4_d h[2]; bf16x8_t v; } vb;
          vb.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr_d)w);
          vb.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr_d)(w + 128));
          acc_o[b][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa[c], vb.v, acc_o[b][dt], 0, 0, 0);
        }
      }
    }
  }

  if constexpr (DIRECT) {
    // ---- npart == 1: merge the four waves through LDS, write bf16 out ----
    // Same arithmetic, in the same order, as multiq_merge_kernel over P = 4;
    // one pass through the scratch per column block.
    float* mg_acc = reinterpret_cast<float*>(lds_all);  // [NWAVES][32][HD]
    float* mg_ml = mg_acc + NWAVES * QCOLS * HEAD_DIM;  // [NWAVES][32][2]
#pragma unroll
    for (int b = 0; b < NQB; ++b) {
      if (b == 1 && !blk1) continue;
      const int bcols = min(ncols - b * QCOLS, QCOLS);
      __syncthreads();  // staging images / the previous pass are done with
      if (lane < bcols) {
        mg_ml[(wave * QCOLS + lane) * 2 + 0] = m_state[b];
        mg_ml[(wave * QCOLS + lane) * 2 + 1] = l_state[b];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = (r & 3) + 8 * (r >> 2) + 4 * half;
        if (qrow >= bcols) continue;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          mg_acc[(wave * QCOLS + qrow) * HEAD_DIM + dt * 32 + col] = acc_o[b][dt][r];
      }
      __syncthreads();
      for (int e = tid; e < bcols * HEAD_DIM; e += NWAVES * 64) {
        const int c = e / HEAD_DIM;
        const int d = e % HEAD_DIM;
        float M = -FLT_MAX;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
          M = fmaxf(M, mg_ml[(w * QCOLS + c) * 2]);
        float L = 0.f, A = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
          const float f = __expf(mg_ml[(w * QCOLS + c) * 2] - M);
          // explicit fma: the merge kernel's loop compiles to fused ops, and
          // both paths must round alike
          L = __builtin_fmaf(f, mg_ml[(w * QCOLS + c) * 2 + 1], L);
          A = __builtin_fmaf(f, mg_acc[(w * QCOLS + c) * HEAD_DIM + d], A);
        }
        const float inv = L > 0.f ? 1.f / L : 0.f;
        const int j = (b * QCOLS + c) / group;
        const int h = (b * QCOLS + c) - j * group;
        out[((long)(q0 + j) * nheads + head0 + h) * HEAD_DIM + d] =
            __float2bfloat16(A * inv);
      }
    }
  } else {
    // ---- per-wave partial store: (m, l) per q col + f32 accumulator ------
    const int P = npart * NWAVES;
    const int pw = part * NWAVES + wave;
#pragma unroll
    for (int b = 0; b < NQB; ++b) {
      if (b == 1 && !blk1) continue;
      if (half == 0 && b * QCOLS + col < ncols) {
        const int j = (b * QCOLS + col) / group;
        const int h = (b * QCOLS + col) - j * group;
        float* ml = part_ml + (((long)(q0 + j) * nheads + head0 + h) * P + pw) * 2;
        ml[0] = m_state[b];
        ml[1] = l_state[b];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = b * QCOLS + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (c >= ncols) continue;
        const int j = c / group;
        const int h = c - j * group;
        float* acc_row =
            part_acc + (((long)(q0 + j) * nheads + head0 + h) * P + pw) * HEAD_DIM;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc_row[dt * 32 + col] = acc_o[b][dt][r];
      }
    }
  }
}

// Reduce the P partials of each computed (token, head) row:
// out = sum_p f_p acc_p / sum_p f_p l_p.  Grid (nseq * max_query_len, nheads):
// rows past a sequence's q_len have no partials and are left alone.
template <int HEAD_DIM>
__global__ void multiq_merge_kernel(
    __hip_bfloat16* __restrict__ out,      // [T, nheads, HD]
    const float* __restrict__ part_acc,    // [T, nheads, P, HD]
    const float* __restrict__ part_ml,     // [T, nheads, P, 2]
    const int* __restrict__ query_start_loc,
    const int nheads,
    const int P,
    const int max_query_len,
    const int total_tokens) {
  const int seq = blockIdx.x / max_query_len;
  const int j = blockIdx.x % max_query_len;
  const int q0 = query_start_loc[seq];
  if (j >= chunk_len(q0, query_start_loc[seq + 1], total_tokens)) return;
  const int head = blockIdx.y;
  const int d = threadIdx.x;
  const long row = (long)(q0 + j) * nheads + head;
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

struct MultiqArgs {
  __hip_bfloat16* out;
  float* part_acc;
  float* part_ml;
  const __hip_bfloat16* q;
  const int* bt;
  const int* qsl;
  const int* sl;
  float scale;
  int nseq, total_tokens, nheads, kvh, head_dim, block_size, max_blocks;
  int max_query_len, npart;
  hipStream_t stream;
};

template <int HEAD_DIM, typename CT, int NQB>
void launch_multiq_nqb(const MultiqArgs& a, const CT* kc, const CT* vc) {
  const int group = a.nheads / a.kvh;
  dim3 grid(a.nseq, a.kvh, a.npart);
  dim3 block(NWAVES * 64);
  if (a.npart == 1) {
    // part_acc / part_ml are not touched on this path
    hipLaunchKernelGGL((paged_multiq_mfma_kernel<HEAD_DIM, CT, NQB, true>), grid,
                       block, 0, a.stream, a.out, a.part_acc, a.part_ml, a.q, kc,
                       vc, a.bt, a.qsl, a.sl, a.scale, a.nheads, a.kvh, group,
                       a.block_size, a.max_blocks, a.total_tokens);
    return;
  }
  hipLaunchKernelGGL((paged_multiq_mfma_kernel<HEAD_DIM, CT, NQB, false>), grid,
                     block, 0, a.stream, a.out, a.part_acc, a.part_ml, a.q, kc,
                     vc, a.bt, a.qsl, a.sl, a.scale, a.nheads, a.kvh, group,
                     a.block_size, a.max_blocks, a.total_tokens);
  hipLaunchKernelGGL(multiq_merge_kernel<HEAD_DIM>,
                     dim3(a.nseq * a.max_query_len, a.nheads), dim3(HEAD_DIM), 0,
                     a.stream, a.out, a.part_acc, a.part_ml, a.qsl, a.nheads,
                     a.npart * NWAVES, a.max_query_len, a.total_tokens);
}

template <typename CT>
void launch_multiq_ct(const MultiqArgs& a, const CT* kc, const CT* vc) {
  const int cols = a.max_query_len * (a.nheads / a.kvh);
  if (a.head_dim == 64 && cols <= QCOLS)
    launch_multiq_nqb<64, CT, 1>(a, kc, vc);
  else if (a.head_dim == 64 && cols <= 2 * QCOLS)
    launch_multiq_nqb<64, CT, 2>(a, kc, vc);
  else if (a.head_dim == 128 && cols <= QCOLS)
    launch_multiq_nqb<128, CT, 1>(a, kc, vc);
  else
    abort();  // the binding checks head_dim and max_query_len * group
}

}  // namespace

void launch_paged_multiq_mfma(__hip_bfloat16* out, float* part_acc,
                              float* part_ml, const __hip_bfloat16* q,
                              const __hip_bfloat16* kc, const __hip_bfloat16* vc,
                              const int* bt, const int* qsl, const int* sl,
                              float scale, int nseq, int total_tokens,
                              int nheads, int kvh, int head_dim, int block_size,
                              int max_blocks, int max_query_len, int npart,
                              hipStream_t stream) {
  launch_multiq_ct<__hip_bfloat16>(
      MultiqArgs{out, part_acc, part_ml, q, bt, qsl, sl, scale, nseq,
                 total_tokens, nheads, kvh, head_dim, block_size, max_blocks,
                 max_query_len, npart, stream},
      kc, vc);
}

void launch_paged_multiq_mfma_fp8(
    __hip_bfloat16* out, float* part_acc, float* part_ml,
    const __hip_bfloat16* q, const unsigned char* kc, const unsigned char* vc,
    const int* bt, const int* qsl, const int* sl, float scale, int nseq,
    int total_tokens, int nheads, int kvh, int head_dim, int block_size,
    int max_blocks, int max_query_len, int npart, hipStream_t stream) {
  launch_multiq_ct<unsigned char>(
      MultiqArgs{out, part_acc, part_ml, q, bt, qsl, sl, scale, nseq,
                 total_tokens, nheads, kvh, head_dim, block_size, max_blocks,
                 max_query_len, npart, stream},
      kc, vc);
}
