// Fused top-k / top-p (nucleus) sampling for 16-bit logits.
//
// One workgroup per row; one launch serves a mixed batch of greedy, plain
// temperature, top-k, top-p and top-k+top-p rows.  Semantics (the torch
// path's, with the sort order made precise):
//   order   tokens by logit descending, ties by lower index first
//   z = logit/T, P = softmax(z) over the whole row, S_j = sum_{i<j} P_i
//   m_p     number of positions with S_j <= top_p
//   c       max(1, min(top_k, m_p)); the kept set is the first c tokens
//   token   argmax over kept of (z_v - log noise_v), ties to the lowest index
//
// No sort and no [N, V] intermediate.  A 16-bit logit has 65 536 distinct
// keys, so the cut is found EXACTLY by a two-level radix select over the
// order-preserving key (high byte, then low byte of the selected bin) with
// 256-bin histograms in LDS.  The row (256 KB at V = 128k) is re-streamed
// from L2 with 16-byte loads for each histogram pass:
//
//   top-p rows only   pass 0  row max (softmax shift)
//   filtered rows     pass 1  high-byte histogram: token count (+ mass)
//                     pass 2  low-byte histogram inside the cut's bin
//   cut inside a tie  pass 3  index-ordered count of the threshold key
//   every row         race    argmax(z - log noise) over the kept set
//
// Unfiltered and greedy rows run the race pass only (what sample_argmax
// does); filtered rows read noise only for their kept tokens.
//
// Determinism: probability mass is accumulated as 64-bit FIXED-POINT
// integers (exp(z - zmax) * 2^40) with integer LDS atomics, so bin sums do
// not depend on arrival order and seeded sampling repeats bit-for-bit.  All
// tokens of one key carry the same integer mass, which makes the cut inside
// the threshold key pure integer arithmetic: token j of that key (index
// order) has prefix mass M + j*m and is kept iff that is <= top_p * Z.
//
// The lowest-index tie rule needs to know WHICH tokens of the threshold key
// are kept when only r of its n are.  Pass 3 counts matches per wave tile
// (64 lanes x 8 contiguous tokens, so tile order == index order), scans the
// tile totals, and one wave re-reads the single tile holding the r-th match.
// It is skipped when r == 0 or r == n.
//
// Every loop is bounded by V; no global atomics, no inter-workgroup traffic.

#include "common.h"
#include <float.h>
#include <limits.h>
#include <stdint.h>

namespace {

typedef unsigned long long u64;
typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE_SIZE;
constexpr int kBins = 256;
constexpr int kTileElems = WAVE_SIZE * 8;  // tokens per wave tile (pass 3)
constexpr int kMaxVocab = 1 << 20;         // V bound: tile table + mass range
constexpr int kMaxSlots = kMaxVocab / kTileElems + 3;  // head + tiles + tail
constexpr float kMassScale = 1099511627776.f;  // 2^40; V * 2^40 < 2^64

template <typename T> DEVINLINE float bits_to_f32(unsigned b);
template <> DEVINLINE float bits_to_f32<__hip_bfloat16>(unsigned b) {
  return __uint_as_float(b << 16);
}
template <> DEVINLINE float bits_to_f32<__half>(unsigned b) {
  return __half2float(__ushort_as_half((unsigned short)b));
}

// 16 raw float bits -> key whose ASCENDING order is DESCENDING value order
// (-0 is folded onto +0 so the two tie, as they do in a value sort).
DEVINLINE unsigned desc_key(unsigned b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? b : 0x7FFFu - b;
}
DEVINLINE unsigned desc_key_to_bits(unsigned d) {
  return (d & 0x8000u) ? d : 0x7FFFu - d;
}

// A row as [head scalars][nvec 16-byte-aligned vectors of 8][tail scalars];
// rows of an odd-V tensor do not start on a 16-byte boundary.
struct RowView {
  const unsigned short* p;
  int head, nvec, tail;
};

DEVINLINE RowView make_view(const void* row, int V) {
  RowView r;
  r.p = reinterpret_cast<const unsigned short*>(row);
  const int mis = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1);
  r.head = mis < V ? mis : V;
  r.nvec = (V - r.head) >> 3;
  r.tail = V - r.head - (r.nvec << 3);
  return r;
}

DEVINLINE const uint4* body_of(const RowView& r) {
  return reinterpret_cast<const uint4*>(r.p + r.head);
}

DEVINLINE unsigned vec_elem(const uint4& v, int e) {
  const unsigned w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}

// Visit the row in no particular order: fv(idx0, vec) for each aligned
// 8-token vector (four loads in flight), fs(idx, bits) for head/tail tokens.
template <typename FV, typename FS>
DEVINLINE void for_each_vec(const RowView& r, FV&& fv, FS&& fs) {
  const int tid = threadIdx.x;
  const uint4* body = body_of(r);
  int j = tid;
  for (; j + 3 * kThreads < r.nvec; j += 4 * kThreads) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = body[j + u * kThreads];
#pragma unroll
    for (int u = 0; u < 4; ++u) fv(r.head + 8 * (j + u * kThreads), v[u]);
  }
  for (; j < r.nvec; j += kThreads) fv(r.head + 8 * j, body[j]);
  if (tid < r.head) fs(tid, (unsigned)r.p[tid]);
  const int t0 = r.head + 8 * r.nvec;
  if (tid < r.tail) fs(t0 + tid, (unsigned)r.p[t0 + tid]);
}

template <typename F>
DEVINLINE void for_each_elem(const RowView& r, F&& f) {
  for_each_vec(
      r,
      [&](int idx0, const uint4& v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f(idx0 + e, vec_elem(v, e));
      },
      f);
}

// Block-wide exclusive prefix sum, one value per thread (integer types, so
// the result is exact).  `scratch` holds kWaves entries and is reusable on
// return.
template <typename I>
DEVINLINE I block_excl_scan(I x, I* scratch) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  I incl = x;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const I o = __shfl_up(incl, off, WAVE_SIZE);
    if (lane >= off) incl += o;
  }
  if (lane == WAVE_SIZE - 1) scratch[wave] = incl;
  __syncthreads();
  I base = 0;
  for (int w = 0; w < wave; ++w) base += scratch[w];
  __syncthreads();
  return base + incl - x;
}

DEVINLINE int wave_reduce_sum_int(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE_SIZE);
  return x;
}

struct Shared {
  unsigned cnt[kBins];       // tokens per bin
  u64 mass[kBins];           // fixed-point probability mass per bin
  unsigned tile[kMaxSlots];  // pass 3: threshold-key matches per wave tile
  unsigned scan32[kWaves];
  u64 scan64[kWaves];
  unsigned red[kWaves];
  int bin_k, bin_p;          // bins where the top-k / top-p budget runs out
  unsigned sel_excl_cnt, sel_cnt;
  u64 sel_excl_mass, sel_mass;
  int slot, rem, bound;
  float best_v[kWaves];
  int best_i[kWaves];
};

struct Cut {
  int bin;        // kBins: budgets outlast the histogram, nothing is cut
  unsigned n;     // tokens in the bin
  u64 mass;       // mass in the bin
};

// Find the first bin in which either budget runs out: `kk` tokens may still
// be kept, `pp` mass may still precede a kept token.  On a hit both budgets
// are reduced by what the bins before it consume, and `before` grows by
// their token count.
DEVINLINE Cut find_cut(Shared& s, bool use_p, unsigned& kk, u64& pp,
                       unsigned& before) {
  const int tid = threadIdx.x;
  const unsigned c = s.cnt[tid];
  const u64 m = use_p ? s.mass[tid] : 0;
  const unsigned ec = block_excl_scan(c, s.scan32);
  const u64 em = use_p ? block_excl_scan(m, s.scan64) : 0;
  if (tid == 0) {
    s.bin_k = kBins;
    s.bin_p = kBins;
  }
  __syncthreads();
  // each condition holds in at most one (non-empty) bin
  if (ec <= kk && kk < ec + c) s.bin_k = tid;
  if (use_p && em <= pp && pp < em + m) s.bin_p = tid;
  __syncthreads();
  const int b = s.bin_k < s.bin_p ? s.bin_k : s.bin_p;
  if (tid == b) {
    s.sel_excl_cnt = ec;
    s.sel_excl_mass = em;
    s.sel_cnt = c;
    s.sel_mass = m;
  }
  __syncthreads();
  Cut cut{b, 0, 0};
  if (b < kBins) {
    kk -= s.sel_excl_cnt;
    if (use_p) pp -= s.sel_excl_mass;
    before += s.sel_excl_cnt;
    cut.n = s.sel_cnt;
    cut.mass = s.sel_mass;
  }
  return cut;
}

// Pass 3 tiles.  Slot 0 is the head, slots 1..ntile the aligned body (64
// lanes x one 8-token vector), the last slot the tail: slot-major then
// lane-major order is index order.  Returns this lane's token count.
DEVINLINE int load_slot(const RowView& r, int slot, int nslots, int lane,
                        unsigned bits[8], int& idx0) {
  if (slot == 0) {
    idx0 = lane;
    if (lane >= r.head) return 0;
    bits[0] = r.p[lane];
    return 1;
  }
  if (slot == nslots - 1) {
    idx0 = r.head + 8 * r.nvec + lane;
    if (lane >= r.tail) return 0;
    bits[0] = r.p[idx0];
    return 1;
  }
  const int j = (slot - 1) * WAVE_SIZE + lane;
  idx0 = r.head + 8 * j;
  if (j >= r.nvec) return 0;
  const uint4 v = body_of(r)[j];
#pragma unroll
  for (int e = 0; e < 8; ++e) bits[e] = vec_elem(v, e);
  return 8;
}

// Index of the r-th (1-based) token whose key equals `thr`, in index order.
DEVINLINE int find_tie_bound(Shared& s, const RowView& view, unsigned thr,
                             unsigned r) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int nslots = (view.nvec + WAVE_SIZE - 1) / WAVE_SIZE + 2;
  if (tid == 0) {
    s.slot = 0;
    s.rem = 0;
    s.bound = INT_MAX;
  }
  for (int slot = wave; slot < nslots; slot += kWaves) {
    unsigned bits[8];
    int idx0;
    const int n = load_slot(view, slot, nslots, lane, bits, idx0);
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += (e < n && desc_key(bits[e]) == thr);
    c = wave_reduce_sum_int(c);
    if (lane == 0) s.tile[slot] = (unsigned)c;
  }
  __syncthreads();
  // which tile holds the r-th match: contiguous runs of tiles per thread
  const int per = (nslots + kThreads - 1) / kThreads;
  const int lo = tid * per < nslots ? tid * per : nslots;
  const int hi = lo + per < nslots ? lo + per : nslots;
  unsigned sum = 0;
  for (int i = lo; i < hi; ++i) sum += s.tile[i];
  unsigned acc = block_excl_scan(sum, s.scan32);
  if (acc < r && r <= acc + sum) {
    for (int i = lo; i < hi; ++i) {
      if (acc + s.tile[i] >= r) {
        s.slot = i;
        s.rem = (int)(r - acc);
        break;
      }
      acc += s.tile[i];
    }
  }
  __syncthreads();
  if (wave == 0) {
    unsigned bits[8];
    int idx0;
    const int n = load_slot(view, s.slot, nslots, lane, bits, idx0);
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += (e < n && desc_key(bits[e]) == thr);
    int incl = c;
#pragma unroll
    for (int off = 1; off < WAVE_SIZE; off <<= 1) {
      const int o = __shfl_up(incl, off, WAVE_SIZE);
      if (lane >= off) incl += o;
    }
    int want = s.rem - (incl - c);  // which of this lane's matches, 1-based
    if (want >= 1 && want <= c) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (e < n && desc_key(bits[e]) == thr && --want == 0)
          s.bound = idx0 + e;
      }
    }
  }
  __syncthreads();
  return s.bound;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_topk_topp_kernel(
    long* __restrict__ out,           // [N]
    int* __restrict__ kept,           // [N] kept-set size, or null
    const T* __restrict__ logits,     // [N, V]
    const float* __restrict__ temps,  // [N] (0 = greedy)
    const float* __restrict__ noise,  // [N, V] Exp(1) draws, or null
    const int* __restrict__ top_k,    // [N] (<=0 or >=V: off)
    const float* __restrict__ top_p,  // [N] (>=1: off)
    const int V) {
  __shared__ Shared s;
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const RowView view = make_view(logits + (long)row * V, V);
  const float* nrow = noise ? noise + (long)row * V : nullptr;
  const float temp = temps[row];
  const bool sample = temp > 0.f && nrow != nullptr;
  const float inv_t = sample ? 1.f / temp : 1.f;
  int k = top_k[row];
  if (k <= 0 || k > V) k = V;
  const float p = top_p[row];
  const bool use_p = sample && p < 1.f;
  const bool filtered = sample && (k < V || use_p);  // block-uniform

  // kept set: key < thr, or key == thr and index <= bound
  unsigned thr = 0x10000u;
  int bound = INT_MAX;
  int nkept = V;

  if (filtered) {
    unsigned kk = (unsigned)k;  // tokens that may still be kept
    u64 pp = ~0ull;             // mass that may still precede a kept token
    unsigned before = 0;        // tokens in bins ahead of the cut
    float zmax = 0.f;
    if (use_p) {
      // pass 0: row max == smallest key
      unsigned mn = 0xFFFFu;
      for_each_elem(view, [&](int, unsigned b) {
        const unsigned d = desc_key(b);
        mn = d < mn ? d : mn;
      });
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(mn, off, WAVE_SIZE);
        mn = o < mn ? o : mn;
      }
      if (lane == 0) s.red[wave] = mn;
      __syncthreads();
      for (int w = 0; w < kWaves; ++w) mn = s.red[w] < mn ? s.red[w] : mn;
      zmax = bits_to_f32<T>(desc_key_to_bits(mn)) * inv_t;
    }
    // fixed-point mass of one token; identical for all tokens of a key
    auto mass_of = [&](unsigned b) -> u64 {
      const float e = __expf(bits_to_f32<T>(b) * inv_t - zmax);
      return e > 0.f ? (u64)(e * kMassScale) : 0ull;
    };

    // pass 1: high byte
    s.cnt[tid] = 0;
    s.mass[tid] = 0;
    __syncthreads();
    for_each_elem(view, [&](int, unsigned b) {
      const unsigned bin = desc_key(b) >> 8;
      atomicAdd(&s.cnt[bin], 1u);
      if (use_p) {
        const u64 m = mass_of(b);
        if (m) atomicAdd(&s.mass[bin], m);
      }
    });
    __syncthreads();
    if (use_p) {
      // budget = top_p * Z in the same fixed point (Z < 2^60: exact enough
      // in f64, and computed identically by every thread)
      const u64 m = s.mass[tid];
      const u64 em = block_excl_scan(m, s.scan64);
      if (tid == kThreads - 1) s.sel_mass = em + m;
      __syncthreads();
      const double z = (double)s.sel_mass;
      pp = (u64)((double)(p > 0.f ? p : 0.f) * z);
      __syncthreads();
    }
    const Cut c1 = find_cut(s, use_p, kk, pp, before);
    if (c1.bin < kBins) {
      // pass 2: low byte inside the selected bin
      const unsigned hi = (unsigned)c1.bin;
      s.cnt[tid] = 0;
      s.mass[tid] = 0;
      __syncthreads();
      for_each_elem(view, [&](int, unsigned b) {
        const unsigned d = desc_key(b);
        if ((d >> 8) != hi) return;
        atomicAdd(&s.cnt[d & 0xFFu], 1u);
        if (use_p) {
          const u64 m = mass_of(b);
          if (m) atomicAdd(&s.mass[d & 0xFFu], m);
        }
      });
      __syncthreads();
      const Cut c2 = find_cut(s, use_p, kk, pp, before);
      if (c2.bin < kBins) {
        thr = (hi << 8) | (unsigned)c2.bin;
        // the n tokens of the threshold key, in index order: token j is kept
        // iff j < kk (top-k) and j * m_e <= pp (its prefix mass <= top_p)
        unsigned r = c2.n < kk ? c2.n : kk;
        const u64 m_e = c2.n ? c2.mass / c2.n : 0;
        if (use_p && m_e) {
          const u64 by_p = pp / m_e + 1;
          if (by_p < r) r = (unsigned)by_p;
        }
        nkept = (int)(before + r);
        if (r == 0) bound = -1;
        else if (r < c2.n) bound = find_tie_bound(s, view, thr, r);
      } else {
        // pass 1 and pass 2 sum the same integers, so this is unreachable;
        // if it were reached, keep the whole bin
        thr = (hi + 1) << 8;
        bound = -1;
        nkept = (int)(before + c1.n);
      }
    }
  }

  // race pass: argmax(z - log noise) over the kept set, ties to lowest index
  float best = -FLT_MAX;
  int best_idx = V;
  auto consider = [&](float v, int idx) {
    if (v > best || (v == best && idx < best_idx)) {
      best = v;
      best_idx = idx;
    }
  };
  if (thr > 0xFFFFu) {
    // nothing cut: stream logits and noise once, as sample_argmax does
    auto one = [&](int idx, unsigned b) {
      float v = bits_to_f32<T>(b);
      if (sample) v = v * inv_t - __logf(nrow[idx]);
      consider(v, idx);
    };
    for_each_vec(
        view,
        [&](int idx0, const uint4& lv) {
          float q[8];
          if (sample) {
            const f32x4u_t a = *reinterpret_cast<const f32x4u_t*>(nrow + idx0);
            const f32x4u_t c =
                *reinterpret_cast<const f32x4u_t*>(nrow + idx0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              q[e] = a[e];
              q[4 + e] = c[e];
            }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = bits_to_f32<T>(vec_elem(lv, e));
            if (sample) v = v * inv_t - __logf(q[e]);
            consider(v, idx0 + e);
          }
        },
        one);
  } else {
    // few tokens survive: noise is read for those only
    for_each_elem(view, [&](int idx, unsigned b) {
      const unsigned d = desc_key(b);
      if (d > thr || (d == thr && idx > bound)) return;
      consider(bits_to_f32<T>(b) * inv_t - __logf(nrow[idx]), idx);
    });
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE_SIZE);
    const int oi = __shfl_xor(best_idx, off, WAVE_SIZE);
    consider(ov, oi);
  }
  if (lane == 0) {
    s.best_v[wave] = best;
    s.best_i[wave] = best_idx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) consider(s.best_v[w], s.best_i[w]);
    out[row] = best_idx;
    if (kept) kept[row] = nkept;
  }
}

}  // namespace

int sample_topk_topp_max_vocab() { return kMaxVocab; }

template <typename T>
void launch_sample_topk_topp(long* out, int* kept, const T* logits,
                             const float* temps, const float* noise,
                             const int* top_k, const float* top_p, int N,
                             int V, hipStream_t stream) {
  hipLaunchKernelGGL(sample_topk_topp_kernel<T>, dim3(N), dim3(kThreads), 0,
                     stream, out, kept, logits, temps, noise, top_k, top_p, V);
}

#define INSTANTIATE_SAMPLE_TOPK_TOPP(T)                                      \
  template void launch_sample_topk_topp<T>(long*, int*, const T*,            \
                                           const float*, const float*,       \
                                           const int*, const float*, int,    \
                                           int, hipStream_t);

INSTANTIATE_SAMPLE_TOPK_TOPP(__hip_bfloat16)
INSTANTIATE_SAMPLE_TOPK_TOPP(__half)
