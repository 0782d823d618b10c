// Token selection of a SAMPLED decode step (decode harness): repetition penalty, temperature, top-k, top-p and the draw, on the
// device, in place of paro_argmax_advance.  The interface it stands in for is the reference's GenerationParams
// (inference/base.py:10-16: temperature = 1.0, top_p, top_k, repetition_penalty), which transformers/generator.py:50-58 hands to HF
// generate() with do_sample = temperature > 0; the order of the steps is HF's processor order (RepetitionPenaltyLogitsProcessor,
// TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, multinomial).
//
// Three launches, ordered by their launch boundaries (no flags or barriers between workgroups), position, token, parameters and
// seed all read from device memory, so one captured graph serves every later step and every later change of parameters:
//   mark    out_tokens[p] = token (advance); the seen set out_tokens[0 .. ctr-1] as one byte per vocabulary entry
//   score   element-wise over a grid: s = penalty(logit) / temperature as fp32, the flag bytes cleared again (no state survives a
//           call: rewinds and multi-turn need no bookkeeping), every workgroup's (max score, lowest index)
//   select  ONE workgroup: max; top-k threshold by radix selection on the monotone 32-bit key of s (8-bit digits, integer counts);
//           top-p threshold the same way on per-digit masses; the draw by narrowing [0, vocab) 16-fold per level in index order.
// Determinism: a mass is exp(s - max) as a 64-bit FIXED-POINT integer (2^-S units, S = min(62 - ceil(log2 vocab), 44), so a sum over
// the whole vocabulary cannot overflow).  Integer sums do not depend on their order, so the LDS histograms may be filled by integer
// atomics and still give the same bits from run to run; there is no float atomic and no float reduction at all.  The comparisons
// against top_p * Z and u * Z are exact integer comparisons (u = m / 2^24: cum > u Z  <=>  cum > floor(m Z / 2^24)).
// Cost: the select workgroup re-reads the fp32 scores (L2-resident: 0.6 MB at 152 k entries) once per digit -- up to nine passes with
// top-k and top-p both on.  Level 0 of a selection puts most entries into a few bins (sign + exponent), so each lane adds into one of
// eight histogram copies (lane & 7), which bounds the same-address serialisation of the LDS atomics.
#include "common.hpp"
#include "sample_rng.hpp"

namespace paro {

constexpr int kScoreTile = 1024;    // vocabulary entries per workgroup of the score pass (256 threads x 4)
constexpr int kSelThreads = 1024;   // the select workgroup: 16 waves
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kHistCopies = 8;
constexpr int64_t kWsHeader = 64;   // 4 stats floats + reserve

struct SampleWs {
  float* stats;                 // {kept count, boundary score, Z, u}
  unsigned long long* bmax;     // [nblk]  (key << 32) | (0xffffffff - index): max = highest score, lowest index
  float* scores;                // [vocab]
  unsigned char* flags;         // [vocab] seen set, all zero between calls
  long long nblk;
};

static inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
static inline int64_t score_blocks(int64_t vocab) { return (vocab + kScoreTile - 1) / kScoreTile; }
static inline int64_t ws_bytes(int64_t vocab) { return kWsHeader + align16(score_blocks(vocab) * 8) + align16(vocab * 4) + align16(vocab); }

// fp32 -> 32-bit key with the same order (and back); -0 never occurs (the score pass stores +0)
__device__ __forceinline__ unsigned mono_key(float s) {
  const unsigned b = __builtin_bit_cast(unsigned, s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_score(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// exp(s - max) in [0, 1] as an integer count of 2^-S
__device__ __forceinline__ unsigned long long fixed_mass(float s, float M, int S) {
  const float e = expf(s - M);
  if (!(e >= 0.f)) return 0ull;   // NaN (inf - inf)
  return (unsigned long long)ldexp((double)fminf(e, 1.0f), S);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// ---- launch 1: record the consumed token, flag the seen set ---------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_mark_kernel(const paro_sample_params_t* prm, const long long* tok, const int* pos,
                                                          long long* out_tokens, long long out_len, unsigned char* flags,
                                                          long long vocab, int advance) {
  const int p = *pos;
  const long long tokv = *tok;
  const bool rec = advance && p >= 0 && p < out_len;     // out_tokens[p] = token
  if (prm->repetition_penalty == 1.0f) {                 // nobody reads the seen set
    if (rec && blockIdx.x == 0 && threadIdx.x == 0) out_tokens[p] = tokv;
    return;
  }
  long long n = (long long)p + advance;                  // ctr: seen = out_tokens[0 .. ctr-1], as far as the array reaches
  n = n < 0 ? 0 : (n > out_len ? out_len : n);
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
    long long t;
    if (rec && j == p) { t = tokv; out_tokens[j] = tokv; }   // (read from *token: no other thread's store is waited for)
    else t = out_tokens[j];
    if (t >= 0 && t < vocab) flags[t] = 1;
  }
}

// ---- launch 2: scores ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_score_kernel(const unsigned short* logits, int act_dtype, long long vocab,
                                                           const paro_sample_params_t* prm, SampleWs w) {
  __shared__ unsigned long long wbest[4];
  const float T = prm->temperature, pen = prm->repetition_penalty;
  const long long base = (long long)blockIdx.x * kScoreTile;
  unsigned long long best = 0;
#pragma unroll
  for (int q = 0; q < kScoreTile / 256; ++q) {
    const long long i = base + q * 256 + threadIdx.x;
    if (i < vocab) {
      float l = act_dtype == PARO_DTYPE_F16 ? f16_bits_to_f32(logits[i]) : bf16_bits_to_f32(logits[i]);
      if (w.flags[i]) {
        w.flags[i] = 0;
        l = l > 0.f ? l / pen : l * pen;
      }
      if (T > 0.f) l = l / T;
      if (l == 0.f) l = 0.f;                               // -0 -> +0: equal scores get equal keys
      w.scores[i] = l;
      const unsigned long long c = ((unsigned long long)mono_key(l) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
      best = c > best ? c : best;
    }
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) best = wbest[k] > best ? wbest[k] : best;
    w.bmax[blockIdx.x] = best;
  }
}

// ---- launch 3: thresholds and the draw, one workgroup ----------------------------------------------------------------------
struct SelShared {
  unsigned long long hist[kHistCopies][256];
  unsigned long long hsum[256];
  unsigned long long red[kSelWaves];
  unsigned long long segsum[kSelWaves];
  unsigned long long segcnt[kSelWaves];
  unsigned long long acc, target;
  int digit;
};

// Radix selection over the entries with key >= lower, highest digit first.  MASS = false: the key of the k-th largest entry
// (target = k entries).  MASS = true: the key at which the descending cumulative mass first reaches top_p * (mass of those entries).
template <bool MASS>
__device__ unsigned radix_select(const float* scores, long long vocab, unsigned lower, float M, int S, unsigned long long k, float top_p,
                                 SelShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0, mask = 0;
  unsigned long long acc = 0, target = k;                  // acc: weight of the entries above the current prefix's bucket
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    for (int j = tid; j < kHistCopies * 256; j += kSelThreads) (&sh.hist[0][0])[j] = 0ull;
    __syncthreads();
    for (long long i = tid; i < vocab; i += kSelThreads) {
      const float s = scores[i];
      const unsigned key = mono_key(s);
      if (key >= lower && (key & mask) == prefix) {
        const unsigned long long wgt = MASS ? fixed_mass(s, M, S) : 1ull;
        atomicAdd(&sh.hist[lane & (kHistCopies - 1)][(key >> shift) & 255u], wgt);
      }
    }
    __syncthreads();
    if (tid < 256) {
      unsigned long long t = 0;
#pragma unroll
      for (int c = 0; c < kHistCopies; ++c) t += sh.hist[c][tid];
      sh.hsum[tid] = t;
    }
    __syncthreads();
    if (tid < 64) {                                        // wave 0: lane L owns bins 255 - 4L .. 252 - 4L, highest first
      unsigned long long b[4], loc = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { b[q] = sh.hsum[255 - 4 * lane - q]; loc += b[q]; }
      const unsigned long long inc = wave_incl_scan_u64(loc, lane);
      if (MASS && level == 0) {
        const unsigned long long total = __shfl(inc, 63, 64);
        unsigned long long want = (unsigned long long)((double)top_p * (double)total);
        want = want > total ? total : want;
        target = want < 1ull ? 1ull : want;
      }
      unsigned long long run = acc + inc - loc;
      unsigned long long above = 0;
      int d = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (d < 0) {
          if (run + b[q] >= target) { d = 255 - 4 * lane - q; above = run; }
          else run += b[q];
        }
      }
      const unsigned long long hit = __ballot(d >= 0);
      const int first = hit ? __ffsll((long long)hit) - 1 : 63;
      if (lane == first) {
        sh.digit = d >= 0 ? d : 0;
        sh.acc = d >= 0 ? above : run;
        sh.target = target;
      }
    }
    __syncthreads();
    prefix |= (unsigned)sh.digit << shift;
    mask |= 255u << shift;
    acc = sh.acc;
    target = sh.target;
  }
  return prefix;
}

__global__ __launch_bounds__(kSelThreads) void sample_select_kernel(SampleWs w, long long vocab, const paro_sample_params_t* prm,
                                                                    long long* tok, int* pos, int advance) {
  __shared__ SelShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float T = prm->temperature, top_p = prm->top_p;
  const int top_k = prm->top_k;
  const int p = *pos;
  const unsigned m24 = sample_bits24(prm->seed, (long long)p + advance);
  const float u = (float)m24 * (1.0f / 16777216.0f);

  // the maximum score and its lowest index
  unsigned long long best = 0;
  for (long long i = tid; i < w.nblk; i += kSelThreads) { const unsigned long long c = w.bmax[i]; best = c > best ? c : best; }
  best = wave_max_u64(best);
  if (lane == 0) sh.red[wave] = best;
  __syncthreads();
  best = sh.red[0];
#pragma unroll
  for (int k = 1; k < kSelWaves; ++k) best = sh.red[k] > best ? sh.red[k] : best;
  const float M = key_score((unsigned)(best >> 32));
  long long arg = (long long)(0xffffffffu - (unsigned)best);
  if (arg >= vocab) arg = 0;

  if (!(T > 0.f)) {                                        // temperature 0: the argmax of the penalised scores
    if (tid == 0) {
      w.stats[0] = 1.f; w.stats[1] = M; w.stats[2] = 1.f; w.stats[3] = u;
      *tok = arg;
      if (advance) *pos = p + 1;
    }
    return;
  }

  int lg = 0;
  while ((1ll << lg) < vocab) ++lg;
  const int S = 62 - lg < 44 ? 62 - lg : 44;
  unsigned thr = 0;                                        // kept: key >= thr
  if (top_k > 0 && (long long)top_k < vocab) thr = radix_select<false>(w.scores, vocab, 0u, M, S, (unsigned long long)top_k, 1.f, sh);
  if (top_p < 1.f) thr = radix_select<true>(w.scores, vocab, thr, M, S, 0ull, top_p, sh);

  // the draw: the lowest index whose cumulative kept mass (index order) exceeds floor(m24 * Z / 2^24); [lo, hi) narrows 16-fold
  long long lo = 0, hi = vocab;
  unsigned long long carry = 0, t = 0, Z = 0, kept = 0;
  bool first = true, found = true;
  do {
    const long long seg = (hi - lo + kSelWaves - 1) / kSelWaves;
    const long long a = lo + wave * seg, b = a + seg < hi ? a + seg : hi;
    unsigned long long sum = 0, cnt = 0;
    for (long long i = a + lane; i < b; i += 64) {
      const float s = w.scores[i];
      if (mono_key(s) >= thr) { sum += fixed_mass(s, M, S); ++cnt; }
    }
    sum = wave_sum_u64(sum);
    cnt = wave_sum_u64(cnt);
    if (lane == 0) { sh.segsum[wave] = sum; sh.segcnt[wave] = cnt; }
    __syncthreads();
    if (first) {
#pragma unroll
      for (int k = 0; k < kSelWaves; ++k) { Z += sh.segsum[k]; kept += sh.segcnt[k]; }
      t = (__umul64hi(Z, (unsigned long long)m24) << 40) | ((Z * (unsigned long long)m24) >> 24);
      first = false;
    }
    unsigned long long run = carry;
    int sel = -1;
#pragma unroll
    for (int k = 0; k < kSelWaves; ++k) {
      if (sel < 0) {
        if (run + sh.segsum[k] > t) sel = k;
        else run += sh.segsum[k];
      }
    }
    __syncthreads();                                       // segsum is rewritten by the next level
    if (sel < 0) { found = false; break; }                 // Z == 0 (no finite score): same in every thread
    carry = run;
    const long long na = lo + sel * seg;
    hi = na + seg < hi ? na + seg : hi;
    lo = na;
  } while (hi - lo > 64);

  if (wave == 0) {
    long long chosen = arg;
    if (found) {
      const long long i = lo + lane;
      unsigned long long q = 0;
      if (i < hi) {
        const float s = w.scores[i];
        if (mono_key(s) >= thr) q = fixed_mass(s, M, S);
      }
      const unsigned long long inc = wave_incl_scan_u64(q, lane);
      const unsigned long long hit = __ballot(q > 0ull && carry + inc > t);
      if (hit) chosen = lo + (__ffsll((long long)hit) - 1);
    }
    if (lane == 0) {
      w.stats[0] = (float)kept;
      w.stats[1] = thr ? key_score(thr) : -__builtin_inff();
      w.stats[2] = (float)ldexp((double)Z, -S);
      w.stats[3] = u;
      *tok = chosen;
      if (advance) *pos = p + 1;
    }
  }
}

}  // namespace paro

extern "C" int64_t paro_sample_workspace_bytes(int64_t vocab) {
  if (vocab < 1 || vocab > 0x7fffffff) return -1;
  return paro::ws_bytes(vocab);
}

extern "C" float paro_sample_uniform(uint64_t seed, int64_t ctr) { return paro::sample_uniform(seed, ctr); }

extern "C" int paro_sample_advance(const void* logits, int64_t vocab, int act_dtype, const paro_sample_params_t* params, int64_t* token,
                                   int32_t* pos, int64_t* out_tokens, int64_t out_len, int advance, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  using namespace paro;
  static_assert(sizeof(paro_sample_params_t) == 24, "paro_sample_params_t is 24 bytes");
  if (!logits || !params || !token || !pos || !workspace) return fail(PARO_ERR_INVALID, "null pointer");
  if (vocab < 1 || vocab > 0x7fffffff) return fail(PARO_ERR_INVALID, "vocab out of range (got %lld)", (long long)vocab);
  if (act_dtype != PARO_DTYPE_F16 && act_dtype != PARO_DTYPE_BF16) return fail(PARO_ERR_INVALID, "act_dtype must be f16 or bf16");
  if (advance != 0 && advance != 1) return fail(PARO_ERR_INVALID, "advance must be 0 or 1 (got %d)", advance);
  if (out_tokens && out_len < 0) return fail(PARO_ERR_INVALID, "out_len must not be negative");
  if (workspace_bytes < ws_bytes(vocab)) return fail(PARO_ERR_INVALID, "sample workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)ws_bytes(vocab));
  SampleWs w;
  w.nblk = score_blocks(vocab);
  w.stats = (float*)workspace;
  w.bmax = (unsigned long long*)((char*)workspace + kWsHeader);
  w.scores = (float*)((char*)w.bmax + align16(w.nblk * 8));
  w.flags = (unsigned char*)((char*)w.scores + align16(vocab * 4));
  hipStream_t st = (hipStream_t)stream;
  if (out_tokens && out_len > 0) {
    const int64_t mb = (out_len + 255) / 256;
    hipLaunchKernelGGL(sample_mark_kernel, dim3((unsigned)(mb < 64 ? mb : 64)), dim3(256), 0, st, params, (const long long*)token, (const int*)pos,
                       (long long*)out_tokens, (long long)out_len, w.flags, (long long)vocab, advance);
  }
  hipLaunchKernelGGL(sample_score_kernel, dim3((unsigned)w.nblk), dim3(256), 0, st, (const unsigned short*)logits, act_dtype, (long long)vocab, params, w);
  hipLaunchKernelGGL(sample_select_kernel, dim3(1), dim3(kSelThreads), 0, st, w, (long long)vocab, params, (long long*)token, pos, advance);
  return check_launch("paro_sample_advance");
}
