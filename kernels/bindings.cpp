// Torch extension bindings for the CDNA4 kernels.
// Built in-tree as vllm_tgis_adapter_amd/_C.so by kernels/build.py
// (hipcc --offload-arch=gfx950).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

// launchers (defined in the .hip translation units)
template <typename T>
void launch_rms_norm(T*, const T*, const T*, float, int, int, hipStream_t);
template <typename T>
void launch_fused_add_rms_norm(T*, T*, const T*, float, int, int, hipStream_t);
template <typename T>
void launch_silu_and_mul(T*, const T*, int, int, hipStream_t);
template <typename T>
void launch_rotary_embedding(const long*, T*, T*, const float*, int, int, int,
                             int, hipStream_t);
template <typename T>
void launch_reshape_and_cache(const T*, const T*, T*, T*, const long*, int,
                              int, hipStream_t);
template <typename T>
void launch_paged_decode(T*, const T*, const T*, const T*, const int*,
                         const int*, float, int, int, int, int, int, int,
                         hipStream_t);
template <typename T>
void launch_paged_prefill(T*, const T*, const T*, const T*, const int*,
                          const int*, const int*, float, int, int, int, int,
                          int, int, int, hipStream_t);
void launch_mfma_probe_32(const unsigned short*, const unsigned short*, float*,
                          hipStream_t);
void launch_mfma_probe_16(const unsigned short*, const unsigned short*, float*,
                          hipStream_t);
void launch_paged_prefill_mfma_v2(__hip_bfloat16*, const __hip_bfloat16*,
                                  const __hip_bfloat16*, const __hip_bfloat16*,
                                  const int*, const int*, const int*, float,
                                  int, int, int, int, int, int, int,
                                  hipStream_t);
void launch_paged_prefill_mfma(__hip_bfloat16*, const __hip_bfloat16*,
                               const __hip_bfloat16*, const __hip_bfloat16*,
                               const int*, const int*, const int*, float, int,
                               int, int, int, int, int, int, hipStream_t);
int decode_mfma_num_partitions(int nseq, int kvh, int max_context);
int gemm_skinny_num_ksplit(int N, int K, int M);
void launch_logsoftmax_topk(float*, int*, float*, int*,
                            const __hip_bfloat16*, const long*, int, int,
                            int, hipStream_t);
void launch_gemm_tile(__hip_bfloat16*, const __hip_bfloat16*,
                      const __hip_bfloat16*, int, int, int, hipStream_t);
void launch_xgmi_allreduce(const unsigned long long*, __hip_bfloat16*,
                           const __hip_bfloat16*, long, long, int, int,
                           hipStream_t);
void launch_paged_decode_mfma_fp8(__hip_bfloat16*, float*, float*,
                                  const __hip_bfloat16*, const unsigned char*,
                                  const unsigned char*, const int*,
                                  const int*, float, int, int, int, int, int,
                                  int, int, hipStream_t);
void launch_paged_prefill_mfma_v2_fp8(__hip_bfloat16*, const __hip_bfloat16*,
                                      const unsigned char*,
                                      const unsigned char*, const int*,
                                      const int*, const int*, float, int, int,
                                      int, int, int, int, int, hipStream_t);
void launch_reshape_and_cache_fp8(const __hip_bfloat16*,
                                  const __hip_bfloat16*, unsigned char*,
                                  unsigned char*, const long*, int, int,
                                  hipStream_t);
void launch_gemm_skinny_q(__hip_bfloat16*, float*, const __hip_bfloat16*,
                          const unsigned char*, const float*, int, int, int,
                          int, int, hipStream_t);
int gemm_tile_q_num_ksplit(int M, int N, int K);
void launch_gemm_tile_q(__hip_bfloat16*, float*, const __hip_bfloat16*,
                        const unsigned char*, const float*, int, int, int,
                        int, int, hipStream_t);
void launch_dequant_weight(__hip_bfloat16*, const unsigned char*,
                           const float*, int, int, int, hipStream_t);
void launch_gemm_skinny(__hip_bfloat16*, float*, const __hip_bfloat16*,
                        const __hip_bfloat16*, int, int, int, int,
                        hipStream_t);
void launch_gemm_skinny_gated(__hip_bfloat16*, float*, const __hip_bfloat16*,
                              const __hip_bfloat16*, int, int, int, int,
                              hipStream_t);
void launch_paged_decode_mfma(__hip_bfloat16*, float*, float*,
                              const __hip_bfloat16*, const __hip_bfloat16*,
                              const __hip_bfloat16*, const int*, const int*,
                              float, int, int, int, int, int, int, int,
                              hipStream_t);
void launch_paged_multiq_mfma(__hip_bfloat16*, float*, float*,
                              const __hip_bfloat16*, const __hip_bfloat16*,
                              const __hip_bfloat16*, const int*, const int*,
                              const int*, float, int, int, int, int, int, int,
                              int, int, int, hipStream_t);
void launch_paged_multiq_mfma_fp8(__hip_bfloat16*, float*, float*,
                                  const __hip_bfloat16*, const unsigned char*,
                                  const unsigned char*, const int*, const int*,
                                  const int*, float, int, int, int, int, int,
                                  int, int, int, int, hipStream_t);
template <typename T>
void launch_lora_shrink(float*, const T*, const T*, const int*, int, int, int,
                        hipStream_t);
template <typename T>
void launch_lora_expand(T*, const float*, const T*, const int*, const float*,
                        int, int, int, int, int, hipStream_t);
int lora_sgmv_num_ksplit(int T, int K);
void launch_lora_sgmv_shrink(float*, const __hip_bfloat16*,
                             const __hip_bfloat16*, const int*, int, int, int,
                             int, int, hipStream_t);
void launch_lora_sgmv_expand(__hip_bfloat16*, const float*,
                             const __hip_bfloat16*, const int*, const float*,
                             int, int, int, int, int, int, int, hipStream_t);
template <typename T>
void launch_sample_argmax(long*, const T*, const float*, const float*, int,
                          int, hipStream_t);
template <typename T>
void launch_sample_topk_topp(long*, int*, const T*, const float*,
                             const float*, const int*, const float*, int, int,
                             hipStream_t);
int sample_topk_topp_max_vocab();
void launch_token_bitmap_scatter(unsigned*, const int*, const int*, int, int,
                                 int, int, hipStream_t);
template <typename T>
void launch_logits_edit(T*, const int*, const float*, const unsigned*,
                        const int*, const unsigned*, const int*, int, int, int,
                        int, int, int, hipStream_t);
void launch_moe_gemm(__hip_bfloat16*, const __hip_bfloat16*,
                     const __hip_bfloat16*, const int*, const int*, int, int,
                     int, int, bool, hipStream_t);
int moe_gemm_q_block_m(int R, int E);
void launch_moe_gemm_q(__hip_bfloat16*, const __hip_bfloat16*,
                       const unsigned char*, const float*, const int*,
                       const int*, int, int, int, int, int, bool,
                       hipStream_t);
int moe_dispatch_block_tokens();
template <typename T>
void launch_moe_dispatch(float*, int*, int*, int*, int*, int*, const T*, int,
                         int, int, bool, bool, hipStream_t);
void launch_moe_combine(__hip_bfloat16*, const __hip_bfloat16*, const int*,
                        const float*, int, int, int, hipStream_t);

namespace {

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

template <typename T>
T* ptr(torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}
template <typename T>
const T* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}

#define DISPATCH_FLOATING(DTYPE, BODY)                                   \
  switch (DTYPE) {                                                       \
    case at::ScalarType::BFloat16: {                                     \
      using scalar_t = __hip_bfloat16;                                   \
      BODY;                                                              \
      break;                                                             \
    }                                                                    \
    case at::ScalarType::Half: {                                         \
      using scalar_t = __half;                                           \
      BODY;                                                              \
      break;                                                             \
    }                                                                    \
    case at::ScalarType::Float: {                                        \
      using scalar_t = float;                                            \
      BODY;                                                              \
      break;                                                             \
    }                                                                    \
    default:                                                             \
      TORCH_CHECK(false, "unsupported dtype");                           \
  }

void rms_norm(torch::Tensor out, torch::Tensor input, torch::Tensor weight,
              double eps) {
  const int hidden = input.size(-1);
  const int rows = input.numel() / hidden;
  TORCH_CHECK(input.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  DISPATCH_FLOATING(input.scalar_type(), {
    launch_rms_norm<scalar_t>(ptr<scalar_t>(out), cptr<scalar_t>(input),
                              cptr<scalar_t>(weight), (float)eps, rows, hidden,
                              current_stream());
  });
}

void fused_add_rms_norm(torch::Tensor x, torch::Tensor residual,
                        torch::Tensor weight, double eps) {
  const int hidden = x.size(-1);
  const int rows = x.numel() / hidden;
  TORCH_CHECK(x.is_contiguous() && residual.is_contiguous());
  DISPATCH_FLOATING(x.scalar_type(), {
    launch_fused_add_rms_norm<scalar_t>(
        ptr<scalar_t>(x), ptr<scalar_t>(residual), cptr<scalar_t>(weight),
        (float)eps, rows, hidden, current_stream());
  });
}

void silu_and_mul(torch::Tensor out, torch::Tensor x) {
  const int d = out.size(-1);
  const int rows = out.numel() / d;
  TORCH_CHECK(x.size(-1) == 2 * d);
  TORCH_CHECK(d % 8 == 0, "intermediate size must be a multiple of 8");
  DISPATCH_FLOATING(x.scalar_type(), {
    launch_silu_and_mul<scalar_t>(ptr<scalar_t>(out), cptr<scalar_t>(x), rows,
                                  d, current_stream());
  });
}

void rotary_embedding(torch::Tensor positions, torch::Tensor q,
                      torch::Tensor k, int64_t head_dim,
                      torch::Tensor cos_sin_cache) {
  const int tokens = positions.size(0);
  const int nq = q.size(-1) / head_dim;
  const int nk = k.size(-1) / head_dim;
  TORCH_CHECK(positions.scalar_type() == at::ScalarType::Long);
  TORCH_CHECK(cos_sin_cache.scalar_type() == at::ScalarType::Float);
  DISPATCH_FLOATING(q.scalar_type(), {
    launch_rotary_embedding<scalar_t>(
        positions.data_ptr<long>(), ptr<scalar_t>(q), ptr<scalar_t>(k),
        cos_sin_cache.data_ptr<float>(), tokens, nq, nk, (int)head_dim,
        current_stream());
  });
}

void reshape_and_cache(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                       torch::Tensor v_cache, torch::Tensor slot_mapping) {
  const int tokens = k.size(0);
  const int row_elems = k_cache.size(2) * k_cache.size(3);
  TORCH_CHECK(slot_mapping.scalar_type() == at::ScalarType::Long);
  if (k_cache.scalar_type() == at::ScalarType::Byte) {
    TORCH_CHECK(k.scalar_type() == at::ScalarType::BFloat16,
                "fp8 KV cache takes bf16 K/V inputs");
    TORCH_CHECK(row_elems % 8 == 0);
    launch_reshape_and_cache_fp8(
        reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
        reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
        reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
        slot_mapping.data_ptr<long>(), tokens, row_elems, current_stream());
    return;
  }
  DISPATCH_FLOATING(k.scalar_type(), {
    launch_reshape_and_cache<scalar_t>(
        cptr<scalar_t>(k), cptr<scalar_t>(v), ptr<scalar_t>(k_cache),
        ptr<scalar_t>(v_cache), slot_mapping.data_ptr<long>(), tokens,
        row_elems, current_stream());
  });
}

void paged_attention_decode(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor seq_lens,
                            double scale) {
  const int nseq = q.size(0);
  const int nheads = q.size(1);
  const int head_dim = q.size(2);
  const int kvh = k_cache.size(2);
  const int block_size = k_cache.size(1);
  const int max_blocks = block_tables.size(1);
  TORCH_CHECK(block_tables.scalar_type() == at::ScalarType::Int);
  TORCH_CHECK(seq_lens.scalar_type() == at::ScalarType::Int);
  const int group = nheads / kvh;
  static const bool force_valu = [] {
    const char* e = getenv("VTA_DECODE_VALU");
    return e && e[0] == '1';
  }();
  const bool kv_fp8 = k_cache.scalar_type() == at::ScalarType::Byte;
  if (kv_fp8) {
    TORCH_CHECK(q.scalar_type() == at::ScalarType::BFloat16 &&
                    (head_dim == 64 || head_dim == 128) && group >= 1 &&
                    group <= 8,
                "fp8 KV cache requires the bf16 MFMA decode path");
    const int npart = decode_mfma_num_partitions(nseq, kvh, max_blocks * block_size);
    const int P = npart * 4;
    auto opts = q.options().dtype(at::ScalarType::Float);
    auto part_acc = at::empty({nseq, nheads, P, head_dim}, opts);
    auto part_ml = at::empty({nseq, nheads, P, 2}, opts);
    launch_paged_decode_mfma_fp8(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        part_acc.data_ptr<float>(), part_ml.data_ptr<float>(),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const unsigned char*>(k_cache.data_ptr()),
        reinterpret_cast<const unsigned char*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(), (float)scale,
        nseq, nheads, kvh, head_dim, block_size, max_blocks, npart,
        current_stream());
    return;
  }
  if (!force_valu && q.scalar_type() == at::ScalarType::BFloat16 &&
      (head_dim == 64 || head_dim == 128) && group >= 1 && group <= 8 &&
      nheads == kvh * group && nseq > 0) {
    const int npart = decode_mfma_num_partitions(nseq, kvh, max_blocks * block_size);
    const int P = npart * 4;
    auto opts = q.options().dtype(at::ScalarType::Float);
    auto part_acc = at::empty({nseq, nheads, P, head_dim}, opts);
    auto part_ml = at::empty({nseq, nheads, P, 2}, opts);
    launch_paged_decode_mfma(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        part_acc.data_ptr<float>(), part_ml.data_ptr<float>(),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(k_cache.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(), (float)scale,
        nseq, nheads, kvh, head_dim, block_size, max_blocks, npart,
        current_stream());
    return;
  }
  DISPATCH_FLOATING(q.scalar_type(), {
    launch_paged_decode<scalar_t>(
        ptr<scalar_t>(out), cptr<scalar_t>(q), cptr<scalar_t>(k_cache),
        cptr<scalar_t>(v_cache), block_tables.data_ptr<int>(),
        seq_lens.data_ptr<int>(), (float)scale, nseq, nheads, kvh, head_dim,
        block_size, max_blocks, current_stream());
  });
}

void paged_attention_prefill(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             torch::Tensor block_tables,
                             torch::Tensor query_start_loc,
                             torch::Tensor seq_lens, double scale,
                             int64_t max_query_len) {
  const int nseq = seq_lens.size(0);
  const int nheads = q.size(1);
  const int head_dim = q.size(2);
  const int kvh = k_cache.size(2);
  const int block_size = k_cache.size(1);
  const int max_blocks = block_tables.size(1);
  static const bool force_valu = [] {
    const char* e = getenv("VTA_PREFILL_VALU");
    return e && e[0] == '1';
  }();
  static const bool force_v1 = [] {
    const char* e = getenv("VTA_PREFILL_V1");
    return e && e[0] == '1';
  }();
  if (k_cache.scalar_type() == at::ScalarType::Byte) {
    TORCH_CHECK(q.scalar_type() == at::ScalarType::BFloat16 && head_dim == 128,
                "fp8 KV cache requires the bf16 v2 prefill path (hd=128)");
    launch_paged_prefill_mfma_v2_fp8(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const unsigned char*>(k_cache.data_ptr()),
        reinterpret_cast<const unsigned char*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), query_start_loc.data_ptr<int>(),
        seq_lens.data_ptr<int>(), (float)scale, nseq, nheads, kvh, head_dim,
        block_size, max_blocks, (int)max_query_len, current_stream());
    return;
  }
  if (!force_valu && !force_v1 &&
      q.scalar_type() == at::ScalarType::BFloat16 && head_dim == 128) {
    launch_paged_prefill_mfma_v2(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(k_cache.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), query_start_loc.data_ptr<int>(),
        seq_lens.data_ptr<int>(), (float)scale, nseq, nheads, kvh, head_dim,
        block_size, max_blocks, (int)max_query_len, current_stream());
    return;
  }
  if (!force_valu && q.scalar_type() == at::ScalarType::BFloat16 &&
      (head_dim == 64 || head_dim == 128)) {
    launch_paged_prefill_mfma(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(k_cache.data_ptr()),
        reinterpret_cast<const __hip_bfloat16*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), query_start_loc.data_ptr<int>(),
        seq_lens.data_ptr<int>(), (float)scale, nseq, nheads, kvh, head_dim,
        block_size, max_blocks, (int)max_query_len, current_stream());
    return;
  }
  DISPATCH_FLOATING(q.scalar_type(), {
    launch_paged_prefill<scalar_t>(
        ptr<scalar_t>(out), cptr<scalar_t>(q), cptr<scalar_t>(k_cache),
        cptr<scalar_t>(v_cache), block_tables.data_ptr<int>(),
        query_start_loc.data_ptr<int>(), seq_lens.data_ptr<int>(),
        (float)scale, nseq, nheads, kvh, head_dim, block_size, max_blocks,
        (int)max_query_len, current_stream());
  });
}

// Short query chunks over a long cached context (speculative verify): every
// sequence's q_len * group query rows ride one pass over its KV stream.
// ops.paged_attention_multiq_usable states the shape contract checked here.
void paged_attention_multiq(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables,
                            torch::Tensor query_start_loc,
                            torch::Tensor seq_lens, double scale,
                            int64_t max_query_len) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 3 && k_cache.dim() == 4 &&
                  block_tables.dim() == 2,
              "q [T, heads, hd], caches [nb, bs, kvh, hd], tables [nseq, mb]");
  const int nseq = seq_lens.numel();
  const int total_tokens = q.size(0);
  const int nheads = q.size(1);
  const int head_dim = q.size(2);
  const int kvh = k_cache.size(2);
  const int block_size = k_cache.size(1);
  const int max_blocks = block_tables.size(1);
  const bool kv_fp8 = k_cache.scalar_type() == at::ScalarType::Byte;
  TORCH_CHECK(q.scalar_type() == at::ScalarType::BFloat16 &&
                  out.scalar_type() == at::ScalarType::BFloat16,
              "multiq attention takes bf16 q and out");
  TORCH_CHECK((kv_fp8 || k_cache.scalar_type() == at::ScalarType::BFloat16) &&
                  v_cache.scalar_type() == k_cache.scalar_type(),
              "multiq attention takes bf16 or e4m3 (uint8) KV caches");
  TORCH_CHECK(block_tables.scalar_type() == at::ScalarType::Int &&
              query_start_loc.scalar_type() == at::ScalarType::Int &&
              seq_lens.scalar_type() == at::ScalarType::Int);
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() &&
                  k_cache.is_contiguous() && v_cache.is_contiguous() &&
                  block_tables.is_contiguous() &&
                  query_start_loc.is_contiguous() && seq_lens.is_contiguous(),
              "multiq attention takes contiguous tensors");
  TORCH_CHECK(out.sizes() == q.sizes() && v_cache.sizes() == k_cache.sizes() &&
              k_cache.size(3) == head_dim && block_tables.size(0) == nseq &&
              query_start_loc.numel() == nseq + 1);
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim 64 or 128");
  const int group = kvh > 0 ? nheads / kvh : 0;
  TORCH_CHECK(group >= 1 && group <= 8 && nheads == kvh * group,
              "nheads must be kvh * group with group <= 8");
  // two 32-column blocks at head_dim 64, one at head_dim 128
  TORCH_CHECK(max_query_len >= 1 &&
                  max_query_len * group <= (head_dim == 64 ? 64 : 32),
              "max_query_len * group must be at most 64 (head_dim 64) or 32 "
              "(head_dim 128)");
  if (nseq == 0 || total_tokens == 0) return;

  const int npart = decode_mfma_num_partitions(nseq, kvh, max_blocks * block_size);
  auto opts = q.options().dtype(at::ScalarType::Float);
  const int P = npart * 4;
  // partials only exist on the partitioned path
  const long rows = npart > 1 ? total_tokens : 0;
  auto part_acc = at::empty({rows, nheads, P, head_dim}, opts);
  auto part_ml = at::empty({rows, nheads, P, 2}, opts);
  auto* o = reinterpret_cast<__hip_bfloat16*>(out.data_ptr());
  auto* qp = reinterpret_cast<const __hip_bfloat16*>(q.data_ptr());
  if (kv_fp8) {
    launch_paged_multiq_mfma_fp8(
        o, part_acc.data_ptr<float>(), part_ml.data_ptr<float>(), qp,
        reinterpret_cast<const unsigned char*>(k_cache.data_ptr()),
        reinterpret_cast<const unsigned char*>(v_cache.data_ptr()),
        block_tables.data_ptr<int>(), query_start_loc.data_ptr<int>(),
        seq_lens.data_ptr<int>(), (float)scale, nseq, total_tokens, nheads,
        kvh, head_dim, block_size, max_blocks, (int)max_query_len, npart,
        current_stream());
    return;
  }
  launch_paged_multiq_mfma(
      o, part_acc.data_ptr<float>(), part_ml.data_ptr<float>(), qp,
      reinterpret_cast<const __hip_bfloat16*>(k_cache.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(v_cache.data_ptr()),
      block_tables.data_ptr<int>(), query_start_loc.data_ptr<int>(),
      seq_lens.data_ptr<int>(), (float)scale, nseq, total_tokens, nheads, kvh,
      head_dim, block_size, max_blocks, (int)max_query_len, npart,
      current_stream());
}

// ---- direct-xGMI all-reduce plumbing (E15) --------------------------------
// Raw hipMalloc (NOT the torch caching allocator: hipIpcGetMemHandle needs
// the allocation base).  Returns (device_ptr, ipc_handle_bytes).
std::tuple<int64_t, py::bytes> xar_alloc(int64_t nbytes) {
  void* p = nullptr;
  TORCH_CHECK(hipMalloc(&p, nbytes) == hipSuccess, "xar_alloc failed");
  TORCH_CHECK(hipMemset(p, 0, nbytes) == hipSuccess);
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess);
  hipIpcMemHandle_t h;
  TORCH_CHECK(hipIpcGetMemHandle(&h, p) == hipSuccess,
              "hipIpcGetMemHandle failed");
  return {reinterpret_cast<int64_t>(p),
          py::bytes(reinterpret_cast<const char*>(&h), sizeof(h))};
}

int64_t xar_open(const std::string& handle_bytes) {
  TORCH_CHECK(handle_bytes.size() == sizeof(hipIpcMemHandle_t));
  hipIpcMemHandle_t h;
  memcpy(&h, handle_bytes.data(), sizeof(h));
  void* p = nullptr;
  TORCH_CHECK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) ==
                  hipSuccess,
              "hipIpcOpenMemHandle failed");
  return reinterpret_cast<int64_t>(p);
}

void xgmi_allreduce(torch::Tensor tensor, torch::Tensor bufs, int64_t cap,
                    int64_t rank, int64_t world) {
  TORCH_CHECK(tensor.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(tensor.is_contiguous() && tensor.is_cuda());
  TORCH_CHECK(bufs.scalar_type() == at::ScalarType::Long && bufs.is_cuda());
  TORCH_CHECK(tensor.numel() * 2 <= cap, "tensor exceeds staging capacity");
  launch_xgmi_allreduce(
      reinterpret_cast<const unsigned long long*>(bufs.data_ptr()),
      reinterpret_cast<__hip_bfloat16*>(tensor.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(tensor.data_ptr()),
      tensor.numel(), cap, (int)rank, (int)world, current_stream());
}

void gemm_tile(torch::Tensor y, torch::Tensor x, torch::Tensor w) {
  const int M = x.size(0);
  const int K = x.size(1);
  const int N = w.size(0);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              w.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(M >= 1 && N % 128 == 0 && K % 64 == 0);
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N);
  launch_gemm_tile(reinterpret_cast<__hip_bfloat16*>(y.data_ptr()),
                   reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                   reinterpret_cast<const __hip_bfloat16*>(w.data_ptr()), M, N,
                   K, current_stream());
}

void gemm_skinny(torch::Tensor y, torch::Tensor x, torch::Tensor w) {
  const int M = x.size(0);
  const int K = x.size(1);
  const int N = w.size(0);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              w.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(M >= 1 && N % 128 == 0 && K % 64 == 0);
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N);
  const int KS = gemm_skinny_num_ksplit(N, K, M);
  torch::Tensor part;
  float* pp = nullptr;
  if (KS > 1) {
    part = at::empty({KS, M, N}, x.options().dtype(at::ScalarType::Float));
    pp = part.data_ptr<float>();
  }
  launch_gemm_skinny(reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), pp,
                     reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(w.data_ptr()), M,
                     N, K, KS, current_stream());
}

void gemm_skinny_q(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                   torch::Tensor wscale, int64_t qbits) {
  const int M = x.size(0);
  const int K = x.size(1);
  const int N = wq.size(0);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(wq.scalar_type() == at::ScalarType::Byte ||
              wq.scalar_type() == at::ScalarType::Char);
  TORCH_CHECK(wscale.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(x.is_contiguous() && wq.is_contiguous() &&
              wscale.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(M >= 1 && M <= 64 && N % 128 == 0 && K % 128 == 0);
  TORCH_CHECK(qbits == 8 || qbits == 4);
  TORCH_CHECK(wq.size(1) == (qbits == 8 ? K : K / 2));
  const int KS = gemm_skinny_num_ksplit(N, K, M);
  torch::Tensor part;
  float* pp = nullptr;
  if (KS > 1) {
    part = at::empty({KS, M, N}, x.options().dtype(at::ScalarType::Float));
    pp = part.data_ptr<float>();
  }
  launch_gemm_skinny_q(
      reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), pp,
      reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
      reinterpret_cast<const unsigned char*>(wq.data_ptr()),
      wscale.data_ptr<float>(), (int)qbits, M, N, K, KS, current_stream());
}

static void check_quant_storage(const torch::Tensor& wq,
                                const torch::Tensor& wscale, int64_t qbits,
                                int N, int K) {
  TORCH_CHECK(qbits == 8 || qbits == 4);
  TORCH_CHECK(wq.scalar_type() == at::ScalarType::Byte ||
              wq.scalar_type() == at::ScalarType::Char);
  TORCH_CHECK(wscale.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(wq.is_cuda() && wscale.is_cuda());
  TORCH_CHECK(wq.is_contiguous() && wscale.is_contiguous());
  TORCH_CHECK(N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0);
  TORCH_CHECK(wq.dim() == 2 && wq.size(1) == (qbits == 8 ? K : K / 2));
  TORCH_CHECK(wscale.numel() == (qbits == 8 ? (int64_t)N
                                            : (int64_t)N * (K / 128)));
  // the kernels fetch the packed bytes as 16-byte vectors
  TORCH_CHECK(reinterpret_cast<uintptr_t>(wq.data_ptr()) % 16 == 0);
}

int64_t gemm_tile_q_ksplit(int64_t M, int64_t N, int64_t K) {
  return gemm_tile_q_num_ksplit((int)M, (int)N, (int)K);
}

void gemm_tile_q(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                 torch::Tensor wscale, int64_t qbits) {
  TORCH_CHECK(x.dim() == 2 && y.dim() == 2);
  const int M = x.size(0);
  const int K = x.size(1);
  const int N = wq.size(0);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              y.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(x.is_cuda() && y.is_cuda());
  TORCH_CHECK(x.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(M >= 1);
  check_quant_storage(wq, wscale, qbits, N, K);
  TORCH_CHECK(y.size(0) == M && y.size(1) == N);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0);
  const int KS = gemm_tile_q_num_ksplit(M, N, K);
  torch::Tensor part;
  float* pp = nullptr;
  if (KS > 1) {
    part = at::empty({KS, M, N}, x.options().dtype(at::ScalarType::Float));
    pp = part.data_ptr<float>();
  }
  launch_gemm_tile_q(
      reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), pp,
      reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
      reinterpret_cast<const unsigned char*>(wq.data_ptr()),
      wscale.data_ptr<float>(), (int)qbits, M, N, K, KS, current_stream());
}

void dequant_weight(torch::Tensor out, torch::Tensor wq, torch::Tensor wscale,
                    int64_t qbits) {
  TORCH_CHECK(out.dim() == 2);
  const int N = out.size(0);
  const int K = out.size(1);
  TORCH_CHECK(out.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous());
  TORCH_CHECK(wq.size(0) == N);
  check_quant_storage(wq, wscale, qbits, N, K);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0);
  launch_dequant_weight(
      reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
      reinterpret_cast<const unsigned char*>(wq.data_ptr()),
      wscale.data_ptr<float>(), (int)qbits, N, K, current_stream());
}

void gemm_skinny_gated(torch::Tensor y, torch::Tensor x, torch::Tensor w13) {
  const int M = x.size(0);
  const int K = x.size(1);
  const int I = w13.size(0) / 2;
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              w13.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(x.is_contiguous() && w13.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(M >= 1 && I % 128 == 0 && K % 64 == 0);
  TORCH_CHECK(w13.size(0) % 2 == 0 && w13.size(1) == K);
  TORCH_CHECK(y.size(0) == M && y.size(1) == I);
  const int KS = gemm_skinny_num_ksplit(I, K, M);
  torch::Tensor part;
  float* pp = nullptr;
  if (KS > 1) {
    part = at::empty({KS, 2, M, I}, x.options().dtype(at::ScalarType::Float));
    pp = part.data_ptr<float>();
  }
  launch_gemm_skinny_gated(
      reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), pp,
      reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(w13.data_ptr()), M, I, K, KS,
      current_stream());
}

void lora_bgmv(torch::Tensor out, torch::Tensor x, torch::Tensor a_stack,
               torch::Tensor b_stack, torch::Tensor tmp, torch::Tensor slots,
               torch::Tensor scales, int64_t off) {
  const int Tn = x.size(0);
  const int K = x.size(1);
  const int R = a_stack.size(1);
  const int N = b_stack.size(1);
  const int out_w = out.size(1);
  TORCH_CHECK(out.size(0) == Tn && tmp.size(0) == Tn && tmp.size(1) == R);
  TORCH_CHECK(a_stack.size(2) == K && b_stack.size(2) == R);
  TORCH_CHECK(R <= 64 && K % 8 == 0);
  TORCH_CHECK(off + N <= out_w);
  TORCH_CHECK(slots.scalar_type() == at::ScalarType::Int);
  TORCH_CHECK(tmp.scalar_type() == at::ScalarType::Float &&
              scales.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() &&
              a_stack.is_contiguous() && b_stack.is_contiguous());
  DISPATCH_FLOATING(x.scalar_type(), {
    launch_lora_shrink<scalar_t>(tmp.data_ptr<float>(), cptr<scalar_t>(x),
                                 cptr<scalar_t>(a_stack),
                                 slots.data_ptr<int>(), Tn, R, K,
                                 current_stream());
    launch_lora_expand<scalar_t>(ptr<scalar_t>(out), tmp.data_ptr<float>(),
                                 cptr<scalar_t>(b_stack),
                                 slots.data_ptr<int>(),
                                 scales.data_ptr<float>(), Tn, R, N, out_w,
                                 (int)off, current_stream());
  });
}

// tmp is the shrink's K-split workspace [lora_sgmv_num_ksplit(T, K), T, Rpad]
// f32 with Rpad = R rounded up to 16.  ops.lora_sgmv_usable states the shape
// conditions for callers; the checks here only guard the kernels' indexing.
void lora_sgmv(torch::Tensor out, torch::Tensor x, torch::Tensor a_stack,
               torch::Tensor b_stack, torch::Tensor tmp, torch::Tensor slots,
               torch::Tensor scales, int64_t off) {
  const int Tn = x.size(0);
  const int K = x.size(1);
  const int L = a_stack.size(0);
  const int R = a_stack.size(1);
  const int N = b_stack.size(1);
  const int out_w = out.size(1);
  const int S = lora_sgmv_num_ksplit(Tn, K);
  const int Rpad = (R + 15) / 16 * 16;
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && a_stack.dim() == 3 &&
              b_stack.dim() == 3 && tmp.dim() == 3);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              out.scalar_type() == at::ScalarType::BFloat16 &&
              a_stack.scalar_type() == at::ScalarType::BFloat16 &&
              b_stack.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(slots.scalar_type() == at::ScalarType::Int &&
              tmp.scalar_type() == at::ScalarType::Float &&
              scales.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() &&
              a_stack.is_contiguous() && b_stack.is_contiguous() &&
              tmp.is_contiguous() && slots.is_contiguous() &&
              scales.is_contiguous());
  for (const torch::Tensor& t : {x, out, a_stack, b_stack, tmp})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0);
  TORCH_CHECK(out.size(0) == Tn && slots.numel() == Tn);
  TORCH_CHECK(a_stack.size(2) == K && b_stack.size(0) == L &&
              b_stack.size(2) == R && scales.numel() == L);
  TORCH_CHECK(tmp.size(0) == S && tmp.size(1) == Tn && tmp.size(2) == Rpad);
  TORCH_CHECK(L >= 1 && R >= 1 && R <= 64 && K >= 128 && K % 128 == 0);
  TORCH_CHECK(N >= 32 && N % 32 == 0 && off >= 0 && off % 8 == 0 &&
              out_w % 8 == 0 && off + N <= out_w);
  if (Tn == 0) return;
  launch_lora_sgmv_shrink(tmp.data_ptr<float>(), cptr<__hip_bfloat16>(x),
                          cptr<__hip_bfloat16>(a_stack), slots.data_ptr<int>(),
                          Tn, R, K, L, S, current_stream());
  launch_lora_sgmv_expand(ptr<__hip_bfloat16>(out), tmp.data_ptr<float>(),
                          cptr<__hip_bfloat16>(b_stack), slots.data_ptr<int>(),
                          scales.data_ptr<float>(), Tn, R, N, out_w, (int)off,
                          L, S, current_stream());
}

void moe_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w,
              torch::Tensor seg_off, bool gated) {
  const int T = x.size(0);
  const int K = x.size(1);
  const int E = w.size(0);
  const long wn = w.size(1);
  const int N = gated ? (int)(wn / 2) : (int)wn;
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              w.scalar_type() == at::ScalarType::BFloat16 &&
              y.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(seg_off.scalar_type() == at::ScalarType::Int &&
              seg_off.numel() == E + 1);
  TORCH_CHECK(N % 128 == 0 && K % 64 == 0 && w.size(2) == K);
  TORCH_CHECK(y.size(0) == T && y.size(1) == N);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous());
  if (T == 0) return;
  launch_moe_gemm(reinterpret_cast<__hip_bfloat16*>(y.data_ptr()),
                  reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                  reinterpret_cast<const __hip_bfloat16*>(w.data_ptr()),
                  seg_off.data_ptr<int>(), nullptr, E, N, K, T, gated,
                  current_stream());
}

// moe_gemm on x[src_row] without the copy: y has src_row.numel() rows, x stays
// in token order.  src_row's values index x's rows; moe_dispatch writes them.
void moe_gemm_gather(torch::Tensor y, torch::Tensor x, torch::Tensor w,
                     torch::Tensor seg_off, torch::Tensor src_row,
                     bool gated) {
  const int R = src_row.numel();
  const int K = x.size(1);
  const int E = w.size(0);
  const long wn = w.size(1);
  const int N = gated ? (int)(wn / 2) : (int)wn;
  TORCH_CHECK(x.dim() == 2 && w.dim() == 3 && y.dim() == 2);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              w.scalar_type() == at::ScalarType::BFloat16 &&
              y.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(seg_off.scalar_type() == at::ScalarType::Int &&
              seg_off.numel() == E + 1 && seg_off.is_contiguous());
  TORCH_CHECK(src_row.scalar_type() == at::ScalarType::Int &&
              src_row.is_contiguous());
  TORCH_CHECK(N % 128 == 0 && K % 64 == 0 && w.size(2) == K);
  TORCH_CHECK(y.size(0) == R && y.size(1) == N);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && y.is_contiguous());
  if (R == 0) return;
  TORCH_CHECK(x.size(0) > 0);
  launch_moe_gemm(reinterpret_cast<__hip_bfloat16*>(y.data_ptr()),
                  reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                  reinterpret_cast<const __hip_bfloat16*>(w.data_ptr()),
                  seg_off.data_ptr<int>(), src_row.data_ptr<int>(), E, N, K,
                  R, gated, current_stream());
}

// moe_gemm / moe_gemm_gather on quantized expert stacks: wq [E, rows, K] int8
// with scales [E, rows], or wq [E, rows, K/2] uint8 nibbles with scales
// [E, rows, K/128].  With src_row, y has src_row.numel() rows and x stays in
// token order.
int64_t moe_gemm_q_tile_rows(int64_t R, int64_t E) {
  return moe_gemm_q_block_m((int)R, (int)E);
}

void moe_gemm_q(torch::Tensor y, torch::Tensor x, torch::Tensor wq,
                torch::Tensor wscale, torch::Tensor seg_off,
                c10::optional<torch::Tensor> src_row, bool gated,
                int64_t qbits) {
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 3 && y.dim() == 2);
  TORCH_CHECK(qbits == 8 || qbits == 4);
  const int R = src_row ? (int)src_row->numel() : (int)x.size(0);
  const int K = x.size(1);
  const int E = wq.size(0);
  const long wn = wq.size(1);
  const int N = gated ? (int)(wn / 2) : (int)wn;
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16 &&
              y.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(wq.scalar_type() ==
              (qbits == 8 ? at::ScalarType::Char : at::ScalarType::Byte));
  TORCH_CHECK(wscale.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(seg_off.scalar_type() == at::ScalarType::Int &&
              seg_off.numel() == E + 1 && seg_off.is_contiguous());
  TORCH_CHECK(E >= 1 && N >= 128 && N % 128 == 0 && (!gated || wn == 2L * N));
  TORCH_CHECK(K >= 64 && K % 64 == 0 && (qbits == 8 || K % 128 == 0));
  TORCH_CHECK(wq.size(2) == (qbits == 8 ? K : K / 2));
  TORCH_CHECK(wscale.dim() == (qbits == 8 ? 2 : 3) && wscale.size(0) == E &&
              wscale.size(1) == wn &&
              (qbits == 8 || wscale.size(2) == K / 128));
  TORCH_CHECK(y.size(0) == R && y.size(1) == N);
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && wq.is_cuda() &&
              wscale.is_cuda() && seg_off.is_cuda());
  TORCH_CHECK(x.is_contiguous() && wq.is_contiguous() &&
              wscale.is_contiguous() && y.is_contiguous());
  // 16-byte x / packed-weight vectors, 8-byte y stores
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(wq.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0);
  const int* rows = nullptr;
  if (src_row) {
    TORCH_CHECK(src_row->scalar_type() == at::ScalarType::Int &&
                src_row->is_contiguous() && src_row->is_cuda());
    rows = src_row->data_ptr<int>();
  }
  if (R == 0) return;
  TORCH_CHECK(x.size(0) > 0);
  const int bm = moe_gemm_q_block_m(R, E);
  TORCH_CHECK((long)E * ((R + bm - 1) / bm) <= 65535);
  launch_moe_gemm_q(reinterpret_cast<__hip_bfloat16*>(y.data_ptr()),
                    reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                    reinterpret_cast<const unsigned char*>(wq.data_ptr()),
                    wscale.data_ptr<float>(), seg_off.data_ptr<int>(), rows,
                    (int)qbits, E, N, K, R, gated, current_stream());
}

// Route + dispatch.  hist is the [nblk, E] int32 workspace of the two-kernel
// path (T > moe_dispatch_block_tokens()).  route_only stops after weights and
// ids; the other outputs may then be empty.
void moe_dispatch(torch::Tensor logits, torch::Tensor weights,
                  torch::Tensor ids, torch::Tensor seg_off,
                  torch::Tensor src_row, torch::Tensor pos,
                  c10::optional<torch::Tensor> hist, bool route_only) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_cuda() && logits.is_contiguous());
  const int Tn = logits.size(0);
  const int E = logits.size(1);
  TORCH_CHECK(weights.dim() == 2 && weights.size(0) == Tn);
  const int k = weights.size(1);
  const long pairs = (long)Tn * k;
  TORCH_CHECK(E >= 2 && E <= 64 && k >= 1 && k <= 8 && k <= E);
  TORCH_CHECK(pairs < (1L << 31));
  TORCH_CHECK(weights.scalar_type() == at::ScalarType::Float &&
              weights.is_contiguous());
  TORCH_CHECK(ids.scalar_type() == at::ScalarType::Int &&
              ids.is_contiguous() && ids.numel() == pairs);
  const int nblk =
      (Tn + moe_dispatch_block_tokens() - 1) / moe_dispatch_block_tokens();
  int* hp = nullptr;
  if (!route_only) {
    for (const torch::Tensor& t : {seg_off, src_row, pos})
      TORCH_CHECK(t.scalar_type() == at::ScalarType::Int && t.is_contiguous());
    TORCH_CHECK(seg_off.numel() == E + 1 && src_row.numel() == pairs &&
                pos.numel() == pairs);
    if (nblk > 1) {
      TORCH_CHECK(hist.has_value() &&
                  hist->scalar_type() == at::ScalarType::Int &&
                  hist->is_contiguous() && hist->numel() == (long)nblk * E);
      hp = hist->data_ptr<int>();
    }
  }
  if (Tn == 0) return;
  const bool vec = E % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0;
  DISPATCH_FLOATING(logits.scalar_type(), {
    launch_moe_dispatch<scalar_t>(
        weights.data_ptr<float>(), ids.data_ptr<int>(),
        route_only ? nullptr : seg_off.data_ptr<int>(),
        route_only ? nullptr : src_row.data_ptr<int>(),
        route_only ? nullptr : pos.data_ptr<int>(), hp, cptr<scalar_t>(logits),
        Tn, E, k, vec, route_only, current_stream());
  });
}

void moe_combine(torch::Tensor out, torch::Tensor ye, torch::Tensor pos,
                 torch::Tensor weights) {
  TORCH_CHECK(out.dim() == 2 && ye.dim() == 2 && pos.dim() == 2 &&
              weights.dim() == 2);
  const int Tn = out.size(0);
  const int H = out.size(1);
  const int k = pos.size(1);
  TORCH_CHECK(out.scalar_type() == at::ScalarType::BFloat16 &&
              ye.scalar_type() == at::ScalarType::BFloat16 &&
              pos.scalar_type() == at::ScalarType::Int &&
              weights.scalar_type() == at::ScalarType::Float);
  TORCH_CHECK(out.is_contiguous() && ye.is_contiguous() &&
              pos.is_contiguous() && weights.is_contiguous());
  TORCH_CHECK(H % 8 == 0 && k >= 1 && k <= 8);
  TORCH_CHECK(pos.size(0) == Tn && weights.size(0) == Tn &&
              weights.size(1) == k);
  TORCH_CHECK(ye.size(0) == (long)Tn * k && ye.size(1) == H);
  for (const torch::Tensor& t : {out, ye})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0);
  if (Tn == 0) return;
  launch_moe_combine(ptr<__hip_bfloat16>(out), cptr<__hip_bfloat16>(ye),
                     pos.data_ptr<int>(), weights.data_ptr<float>(), Tn, H, k,
                     current_stream());
}

void sample_argmax(torch::Tensor out, torch::Tensor logits,
                   torch::Tensor temps, c10::optional<torch::Tensor> noise) {
  const int N = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(out.scalar_type() == at::ScalarType::Long && out.size(0) == N);
  TORCH_CHECK(temps.scalar_type() == at::ScalarType::Float && temps.size(0) == N);
  TORCH_CHECK(logits.is_contiguous());
  const float* np_ = nullptr;
  if (noise.has_value()) {
    TORCH_CHECK(noise->scalar_type() == at::ScalarType::Float &&
                noise->is_contiguous() && noise->size(0) == N &&
                noise->size(1) == V);
    np_ = noise->data_ptr<float>();
  }
  DISPATCH_FLOATING(logits.scalar_type(), {
    launch_sample_argmax<scalar_t>(out.data_ptr<long>(),
                                   cptr<scalar_t>(logits),
                                   temps.data_ptr<float>(), np_, N, V,
                                   current_stream());
  });
}

void sample_topk_topp(torch::Tensor out, torch::Tensor logits,
                      torch::Tensor temps, c10::optional<torch::Tensor> noise,
                      torch::Tensor top_k, torch::Tensor top_p,
                      c10::optional<torch::Tensor> kept) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_cuda() && logits.is_contiguous());
  const int N = logits.size(0);
  const long V = logits.size(1);
  const auto dev = logits.device();
  TORCH_CHECK(V >= 1 && V <= sample_topk_topp_max_vocab(),
              "vocab out of range for sample_topk_topp");
  TORCH_CHECK(out.scalar_type() == at::ScalarType::Long && out.dim() == 1 &&
              out.size(0) == N && out.is_contiguous() && out.device() == dev);
  TORCH_CHECK(temps.scalar_type() == at::ScalarType::Float &&
              temps.dim() == 1 && temps.size(0) == N &&
              temps.is_contiguous() && temps.device() == dev);
  TORCH_CHECK(top_k.scalar_type() == at::ScalarType::Int && top_k.dim() == 1 &&
              top_k.size(0) == N && top_k.is_contiguous() &&
              top_k.device() == dev);
  TORCH_CHECK(top_p.scalar_type() == at::ScalarType::Float &&
              top_p.dim() == 1 && top_p.size(0) == N &&
              top_p.is_contiguous() && top_p.device() == dev);
  const float* np_ = nullptr;
  if (noise.has_value()) {
    TORCH_CHECK(noise->scalar_type() == at::ScalarType::Float &&
                noise->is_contiguous() && noise->dim() == 2 &&
                noise->size(0) == N && noise->size(1) == V &&
                noise->device() == dev);
    np_ = noise->data_ptr<float>();
  }
  int* kp = nullptr;
  if (kept.has_value()) {
    TORCH_CHECK(kept->scalar_type() == at::ScalarType::Int &&
                kept->dim() == 1 && kept->size(0) == N &&
                kept->is_contiguous() && kept->device() == dev);
    kp = kept->data_ptr<int>();
  }
  if (N == 0) return;
  switch (logits.scalar_type()) {
    case at::ScalarType::BFloat16:
      launch_sample_topk_topp<__hip_bfloat16>(
          out.data_ptr<long>(), kp, cptr<__hip_bfloat16>(logits),
          temps.data_ptr<float>(), np_, top_k.data_ptr<int>(),
          top_p.data_ptr<float>(), N, (int)V, current_stream());
      break;
    case at::ScalarType::Half:
      launch_sample_topk_topp<__half>(
          out.data_ptr<long>(), kp, cptr<__half>(logits),
          temps.data_ptr<float>(), np_, top_k.data_ptr<int>(),
          top_p.data_ptr<float>(), N, (int)V, current_stream());
      break;
    default:
      TORCH_CHECK(false, "sample_topk_topp serves bf16 / f16 logits only");
  }
}

// token bitmaps: int32 [slots, W] holding the uint32 words' bits, 16-byte rows
void check_token_bitmap(const torch::Tensor& bm, const c10::Device& dev) {
  TORCH_CHECK(bm.scalar_type() == at::ScalarType::Int && bm.dim() == 2 &&
              bm.is_contiguous() && bm.device() == dev &&
              bm.size(1) % 4 == 0 && bm.size(0) < (1 << 24),
              "token bitmap must be contiguous int32 [slots, W], W % 4 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(bm.data_ptr()) % 16 == 0);
}

void check_int_list(const torch::Tensor& t, long n, const c10::Device& dev) {
  TORCH_CHECK(t.scalar_type() == at::ScalarType::Int && t.dim() == 1 &&
              t.size(0) == n && t.is_contiguous() && t.device() == dev);
}

void token_bitmap_scatter(torch::Tensor bitmap, torch::Tensor slots,
                          torch::Tensor tokens, int64_t vocab) {
  TORCH_CHECK(bitmap.is_cuda());
  const auto dev = bitmap.device();
  check_token_bitmap(bitmap, dev);
  const long P = slots.numel();
  check_int_list(slots, P, dev);
  check_int_list(tokens, P, dev);
  TORCH_CHECK(vocab >= 0 && vocab <= bitmap.size(1) * 32 && P < (1L << 31),
              "vocab exceeds the bitmap row");
  if (P == 0 || bitmap.size(0) == 0) return;
  launch_token_bitmap_scatter(ptr<unsigned>(bitmap), slots.data_ptr<int>(),
                              tokens.data_ptr<int>(), (int)P,
                              (int)bitmap.size(0), (int)bitmap.size(1),
                              (int)vocab, current_stream());
}

void logits_edit(torch::Tensor logits, torch::Tensor rows,
                 torch::Tensor penalties, c10::optional<torch::Tensor> seen,
                 c10::optional<torch::Tensor> seen_slots,
                 c10::optional<torch::Tensor> allow,
                 c10::optional<torch::Tensor> allow_slots) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_cuda() && logits.is_contiguous());
  const auto dev = logits.device();
  const long N = logits.size(0);
  const long V = logits.size(1);
  TORCH_CHECK(V % 8 == 0 && V < (1L << 30) && N < (1L << 31),
              "logits_edit needs V % 8 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0);
  const long E = rows.numel();
  check_int_list(rows, E, dev);
  TORCH_CHECK(penalties.scalar_type() == at::ScalarType::Float &&
              penalties.dim() == 1 && penalties.size(0) == E &&
              penalties.is_contiguous() && penalties.device() == dev);
  const long W = ((V + 31) / 32 + 3) / 4 * 4;
  const unsigned* sp = nullptr;
  const unsigned* ap = nullptr;
  const int* ssp = nullptr;
  const int* asp = nullptr;
  int n_seen = 0, n_allow = 0;
  if (seen.has_value()) {
    TORCH_CHECK(seen_slots.has_value(), "seen needs seen_slots");
    check_token_bitmap(*seen, dev);
    check_int_list(*seen_slots, E, dev);
    TORCH_CHECK(seen->size(1) == W, "seen bitmap width does not fit V");
    sp = cptr<unsigned>(*seen);
    ssp = seen_slots->data_ptr<int>();
    n_seen = (int)seen->size(0);
  }
  if (allow.has_value()) {
    TORCH_CHECK(allow_slots.has_value(), "allow needs allow_slots");
    check_token_bitmap(*allow, dev);
    check_int_list(*allow_slots, E, dev);
    TORCH_CHECK(allow->size(1) == W, "allow bitmap width does not fit V");
    ap = cptr<unsigned>(*allow);
    asp = allow_slots->data_ptr<int>();
    n_allow = (int)allow->size(0);
  }
  if (E == 0 || N == 0 || (n_seen == 0 && n_allow == 0)) return;
  DISPATCH_FLOATING(logits.scalar_type(), {
    launch_logits_edit<scalar_t>(ptr<scalar_t>(logits), rows.data_ptr<int>(),
                                 penalties.data_ptr<float>(), sp, ssp, ap, asp,
                                 (int)E, (int)N, (int)V, (int)W, n_seen,
                                 n_allow, current_stream());
  });
}

void logsoftmax_topk(torch::Tensor topv, torch::Tensor topi,
                     torch::Tensor chosen_lp, torch::Tensor ranks,
                     torch::Tensor logits, torch::Tensor chosen) {
  const int N = logits.size(0);
  const int V = logits.size(1);
  const int K = topv.size(1);
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::BFloat16 &&
              logits.is_contiguous());
  TORCH_CHECK(V % 8 == 0, "vocab must be a multiple of 8");
  TORCH_CHECK(K <= 16, "K <= 16");
  TORCH_CHECK(topv.scalar_type() == at::ScalarType::Float &&
              topi.scalar_type() == at::ScalarType::Int &&
              topv.is_contiguous() && topi.is_contiguous() &&
              topi.size(1) == K && topv.size(0) == N && topi.size(0) == N);
  TORCH_CHECK(chosen_lp.scalar_type() == at::ScalarType::Float &&
              chosen_lp.size(0) == N);
  TORCH_CHECK(ranks.scalar_type() == at::ScalarType::Int && ranks.size(0) == N);
  TORCH_CHECK(chosen.scalar_type() == at::ScalarType::Long &&
              chosen.is_contiguous() && chosen.size(0) == N);
  launch_logsoftmax_topk(
      topv.data_ptr<float>(), topi.data_ptr<int>(),
      chosen_lp.data_ptr<float>(), ranks.data_ptr<int>(),
      reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
      chosen.data_ptr<long>(), N, V, K, current_stream());
}

void mfma_probe(torch::Tensor a, torch::Tensor b, torch::Tensor d, int64_t shape) {
  TORCH_CHECK(a.scalar_type() == at::ScalarType::BFloat16);
  auto* ap = reinterpret_cast<const unsigned short*>(a.data_ptr());
  auto* bp = reinterpret_cast<const unsigned short*>(b.data_ptr());
  auto* dp = d.data_ptr<float>();
  if (shape == 32)
    launch_mfma_probe_32(ap, bp, dp, current_stream());
  else
    launch_mfma_probe_16(ap, bp, dp, current_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("mfma_probe", &mfma_probe, "MFMA fragment layout probe");
  m.def("rms_norm", &rms_norm, "fused RMSNorm (CDNA4)");
  m.def("fused_add_rms_norm", &fused_add_rms_norm,
        "in-place residual-add + RMSNorm (CDNA4)");
  m.def("silu_and_mul", &silu_and_mul, "SwiGLU activation (CDNA4)");
  m.def("rotary_embedding", &rotary_embedding, "NeoX rotary, in place (CDNA4)");
  m.def("reshape_and_cache", &reshape_and_cache, "paged KV cache write (CDNA4)");
  m.def("paged_attention_decode", &paged_attention_decode,
        "paged decode attention (CDNA4)");
  m.def("paged_attention_prefill", &paged_attention_prefill,
        "paged causal prefill attention (CDNA4)");
  m.def("paged_attention_multiq", &paged_attention_multiq,
        "paged causal attention for short query chunks, one KV pass per "
        "(sequence, KV head) (CDNA4 MFMA)");
  m.def("xar_alloc", &xar_alloc,
        "raw hipMalloc + IPC handle for the xGMI all-reduce staging buffer");
  m.def("xar_open", &xar_open, "open a peer's IPC handle -> device pointer");
  m.def("xgmi_allreduce", &xgmi_allreduce,
        "in-place one-shot all-reduce over peer-mapped xGMI buffers");
  m.def("gemm_tile", &gemm_tile,
        "128x128-tile glds-staged bf16 GEMM for decode batches (CDNA4)");
  m.def("gemm_skinny_q", &gemm_skinny_q,
        "weight-only-quantized (int8 / int4-g128) skinny decode GEMM");
  m.def("gemm_tile_q", &gemm_tile_q,
        "weight-only-quantized (int8 / int4-g128) tile GEMM, M > 64");
  m.def("gemm_tile_q_ksplit", &gemm_tile_q_ksplit,
        "K-split count gemm_tile_q uses for (M, N, K)");
  m.def("dequant_weight", &dequant_weight,
        "one-pass int8 / int4-g128 -> bf16 weight dequantisation");
  m.def("gemm_skinny", &gemm_skinny,
        "skinny decode GEMM y = x @ w^T, M <= 64 (CDNA4 MFMA)");
  m.def("gemm_skinny_gated", &gemm_skinny_gated,
        "fused gate/up skinny GEMM + SiLU-mul, M <= 64 (CDNA4 MFMA)");
  m.def("moe_gemm", &moe_gemm,
        "grouped MoE GEMM over expert segments (CDNA4 MFMA)");
  m.def("moe_gemm_gather", &moe_gemm_gather,
        "grouped MoE GEMM that gathers its x rows through src_row");
  m.def("moe_gemm_q", &moe_gemm_q,
        "grouped MoE GEMM on int8 / int4-g128 expert weights (CDNA4 MFMA)");
  m.def("moe_gemm_q_tile_rows", &moe_gemm_q_tile_rows,
        "x rows per workgroup moe_gemm_q uses for (R, E)");
  m.def("moe_dispatch", &moe_dispatch,
        "MoE top-k routing + stable counting-sort dispatch (CDNA4)");
  m.def("moe_dispatch_block_tokens", &moe_dispatch_block_tokens,
        "tokens per moe_dispatch workgroup (one launch up to this T)");
  m.def("moe_combine", &moe_combine,
        "weighted f32 combine of the experts' sorted output rows (CDNA4)");
  m.def("logsoftmax_topk", &logsoftmax_topk,
        "fused log-softmax + top-K + sampled-token rank (one HBM pass)");
  m.def("sample_argmax", &sample_argmax,
        "fused temperature/gumbel-race sampling + greedy argmax (CDNA4)");
  m.def("sample_topk_topp", &sample_topk_topp,
        "fused top-k / top-p sampling, radix-select cut + race (CDNA4)");
  m.def("sample_topk_topp_max_vocab", &sample_topk_topp_max_vocab,
        "largest vocab sample_topk_topp serves");
  m.def("token_bitmap_scatter", &token_bitmap_scatter,
        "OR (slot, token) pairs into a per-slot token bitmap");
  m.def("logits_edit", &logits_edit,
        "bitmap-driven repetition penalty + allow mask, in place (CDNA4)");
  m.def("lora_bgmv", &lora_bgmv,
        "batched multi-LoRA shrink+expand for mixed-adapter batches (CDNA4)");
  m.def("lora_sgmv", &lora_sgmv,
        "segmented multi-LoRA shrink+expand for prefill batches (CDNA4 MFMA)");
  m.def("lora_sgmv_num_ksplit", &lora_sgmv_num_ksplit,
        "K-split of the lora_sgmv shrink grid (pure function of shapes)");
}
