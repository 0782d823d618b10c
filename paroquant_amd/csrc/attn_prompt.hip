// Attention of a prompt CONTINUATION (decode harness, ABI v20): `rows` new query rows at positions pos0 .. pos0 + rows - 1 attend causally
// to the decode caches -- the positions earlier calls left there and each other (paro_prompt_qkv_post has already written this chunk's K / V at
// pos0 + t).  It is what lets the harness add a chat turn to the context it holds, run a long prompt in chunks, or rewind, without
// re-running the prefix: the prompt pass' SDPA sees only the new rows, the decode kernel (attn.hip) only one.
//
// Grid = (query blocks, KV heads); one 256-thread workgroup per (block, KV head).  Its 64 MFMA rows are (query row, query head of the group)
// pairs -- row r = t * n_rep + j, 64 / n_rep query rows per block -- so the K / V bytes of a KV head are staged ONCE for all the query heads
// that read them.  Wave w owns rows 16 w .. 16 w + 15.  The workgroup walks the cache in 64-position tiles from position 0 to its last row's
// position (tiles wholly above the causal diagonal are not visited; a wave skips the tiles above its own rows), staging each tile in LDS
// while the next one is in flight in registers:
//   K tile [64 pos][hd]     B fragments of S = Q K^T: lane (kb, mm) reads dims 32 i + 8 kb .. + 7 of position 16 t + mm
//   V tile [hd][64 pos]     B fragments of O = P V:   lane (kb, mm) reads positions 32 i + 8 kb .. + 7 of dim 16 t + mm
// Scores and P V are mfma_f32_16x16x32 (f16 / bf16); the soft-max is the online one in fp32 (base 2, the scale folded into log2 e / sqrt(hd)):
// at every tile the running output and sum are multiplied by 2^(m_old - m_new) -- exactly 1 when the maximum did not move, no threshold.
// P is rounded to the activation dtype for the MFMA (through a per-wave LDS block: the D layout of S is not the A layout of P V), the
// output is divided by the fp32 sum and rounded once.  No atomics and no cross-workgroup reduction: the same bits on every run.
// Cache positions >= pos0 + rows are never read: K rows there are staged as zeros, V words are loaded element-wise at the boundary.
#include "common.hpp"

namespace paro {

constexpr int kApTile = 64;   // cache positions per staged tile
constexpr int kApRows = 64;   // MFMA rows per workgroup (4 waves x 16)

template <typename AT, int HD>
__global__ __launch_bounds__(256) void attn_prompt_kernel(const unsigned short* __restrict__ q, const unsigned short* __restrict__ kcache,
                                                          const unsigned short* __restrict__ vcache, unsigned short* __restrict__ out, int rows,
                                                          int pos0, int Hq, int n_rep, int qb_rows, int T_max, float scale_log2) {
  typedef Act<AT> A;
  typedef typename A::vec8 vec8;
  constexpr int KP = HD + 8;        // row pitches (elements) of the LDS tiles: 16 B of padding spreads a fragment's 16 rows over the banks
  constexpr int VP = kApTile + 8;
  constexpr int PP = kApTile + 8;
  constexpr int KS = HD / 32;       // MFMA k-steps of a score
  constexpr int DT = HD / 16;       // 16-dim output tiles
  constexpr int KC = kApTile * HD / 8 / 256;   // 16-byte K chunks per thread and tile
  constexpr int VC = HD * kApTile / 8 / 256;   // 16-byte V chunks per thread and tile
  __shared__ __attribute__((aligned(16))) unsigned short ks[kApTile * KP];
  __shared__ __attribute__((aligned(16))) unsigned short vs[HD * VP];
  __shared__ __attribute__((aligned(16))) unsigned short ps[4 * 16 * PP];   // [wave][row][position] rounded probabilities
  constexpr float kNegInf = -__builtin_inff();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kb = lane >> 4, mm = lane & 15;
  const int g = blockIdx.y;
  const int t0 = blockIdx.x * qb_rows;                // first query row of the block
  const int nt = min(qb_rows, rows - t0);             // its query rows
  const int kend = pos0 + rows;                       // first cache position never read
  const int64_t kbase = (int64_t)g * T_max * HD;      // this KV head's K rows
  const int64_t vbase = (int64_t)g * HD * T_max;      // ... and V rows

  // the A operand of the scores: MFMA row mm of this wave = workgroup row 16 wave + mm -> (query row, head); padding rows are zero
  vec8 qa[KS];
  {
    const int ra = 16 * wave + mm, ta = ra / n_rep, ja = ra - ta * n_rep;
    const bool va = ta < nt;
    const unsigned short* qr = q + (((int64_t)(t0 + (va ? ta : 0)) * Hq + g * n_rep + ja) * HD);
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const u32x4 w = va ? *(const u32x4*)(qr + 32 * i + 8 * kb) : u32x4{0u, 0u, 0u, 0u};
      qa[i] = __builtin_bit_cast(vec8, w);
    }
  }
  // the D rows 4 kb + r this lane holds: their query row's absolute position (padding rows take the block's first, a valid one)
  int qpos[4], td[4], jd[4];
  bool vd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rd = 16 * wave + 4 * kb + r;
    td[r] = rd / n_rep;
    jd[r] = rd - td[r] * n_rep;
    vd[r] = td[r] < nt;
    qpos[r] = pos0 + t0 + (vd[r] ? td[r] : 0);
  }
  const int w_first = (16 * wave) / n_rep;            // this wave's first query row
  const int wave_qmax = w_first < nt ? pos0 + t0 + min((16 * wave + 15) / n_rep, nt - 1) : -1;   // its last position (-1: no rows)
  const int ntiles = (pos0 + t0 + nt - 1) / kApTile + 1;

  u32x4 kr[KC], vr[VC];
  auto fetch = [&](int tile) {
    const int p0 = tile * kApTile;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int e = tid + 256 * c, p = p0 + e / (HD / 8), d8 = e % (HD / 8);
      kr[c] = p < kend ? *(const u32x4*)(kcache + kbase + (int64_t)p * HD + d8 * 8) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int c = 0; c < VC; ++c) {
      const int e = tid + 256 * c, d = e / (kApTile / 8), p = p0 + (e % (kApTile / 8)) * 8;
      const unsigned short* src = vcache + vbase + (int64_t)d * T_max + p;
      if (p + 8 <= kend) {
        vr[c] = *(const u32x4*)src;                   // T_max and p are multiples of 8: 16-byte aligned
      } else {                                        // the tile holding the last position: element by element up to it
        unsigned w[4] = {0u, 0u, 0u, 0u};
        for (int x = 0; x < 8 && p + x < kend; ++x) w[x >> 1] |= (unsigned)src[x] << (16 * (x & 1));
        vr[c] = u32x4{w[0], w[1], w[2], w[3]};
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int e = tid + 256 * c;
      *(u32x4*)(ks + (e / (HD / 8)) * KP + (e % (HD / 8)) * 8) = kr[c];
    }
#pragma unroll
    for (int c = 0; c < VC; ++c) {
      const int e = tid + 256 * c;
      *(u32x4*)(vs + (e / (kApTile / 8)) * VP + (e % (kApTile / 8)) * 8) = vr[c];
    }
  };

  float m[4], l[4];
  f32x4 o[DT];
#pragma unroll
  for (int r = 0; r < 4; ++r) m[r] = kNegInf, l[r] = 0.f;
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  unsigned short* pw = ps + wave * 16 * PP;

  fetch(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    stage();
    __syncthreads();
    if (tile + 1 < ntiles) fetch(tile + 1);           // in flight while this tile is consumed
    const int p0 = tile * kApTile;
    if (p0 <= wave_qmax) {
      // S = Q K^T: D[row 4 kb + r][col mm] of 16-position tile t; positions above a row's diagonal are -inf (never a product with them)
      float s[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KS; ++i) d = A::mfma(qa[i], *(const vec8*)(ks + (16 * t + mm) * KP + 32 * i + 8 * kb), d);
        const int kp = p0 + 16 * t + mm;
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = kp <= qpos[r] ? d[r] * scale_log2 : kNegInf;
      }
      // online soft-max: a row's 64 scores live in the 16 lanes of its lane row kb (4 tiles each)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x));
        const float mn = fmaxf(m[r], mx);
        const float mu = mn == kNegInf ? 0.f : mn;    // (a row with nothing seen yet: no inf - inf)
        const float alpha = __builtin_amdgcn_exp2f(m[r] - mu);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float p = __builtin_amdgcn_exp2f(s[t][r] - mu);
          sum += p;
          pw[(4 * kb + r) * PP + 16 * t + mm] = A::from_f32(p);
        }
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) sum += __shfl_xor(sum, x);
        l[r] = __builtin_fmaf(l[r], alpha, sum);
        m[r] = mn;
#pragma unroll
        for (int t = 0; t < DT; ++t) o[t][r] *= alpha;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the wave reads back what its own lanes wrote (LDS is in order per wave)
      __builtin_amdgcn_wave_barrier();
      // O += P V: A = P (row mm, positions 32 i + 8 kb ..), B = V (dim 16 t + mm, the same positions)
      vec8 pa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) pa[i] = *(const vec8*)(pw + mm * PP + 32 * i + 8 * kb);
#pragma unroll
      for (int t = 0; t < DT; ++t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) o[t] = A::mfma(pa[i], *(const vec8*)(vs + (16 * t + mm) * VP + 32 * i + 8 * kb), o[t]);
      }
    }
    __syncthreads();                                  // the tiles are overwritten next
  }

  // out[t][head][d] = O / l, rounded once
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (!vd[r]) continue;
    const float inv = 1.0f / l[r];
    unsigned short* orow = out + (((int64_t)(t0 + td[r]) * Hq + g * n_rep + jd[r]) * HD);
#pragma unroll
    for (int t = 0; t < DT; ++t) orow[16 * t + mm] = A::from_f32(o[t][r] * inv);
  }
}

template <typename AT, int HD>
static void launch_attn_prompt(const void* q, const void* kc, const void* vc, void* out, int rows, int pos0, int Hq, int Hkv, int T_max,
                               hipStream_t st) {
  const int n_rep = Hq / Hkv, qb = kApRows / n_rep;
  const dim3 grid((unsigned)((rows + qb - 1) / qb), (unsigned)Hkv);
  const float scale_log2 = 1.4426950408889634f / __builtin_sqrtf((float)HD);
  hipLaunchKernelGGL((attn_prompt_kernel<AT, HD>), grid, dim3(256), 0, st, (const unsigned short*)q, (const unsigned short*)kc,
                     (const unsigned short*)vc, (unsigned short*)out, rows, pos0, Hq, n_rep, qb, T_max, scale_log2);
}

}  // namespace paro

extern "C" int paro_attn_prompt(const void* q, const void* kcache, const void* vcache, void* out, int64_t rows, int pos0, int n_heads,
                                int n_kv_heads, int head_dim, int max_positions, int act_dtype, void* stream) {
  using namespace paro;
  if (head_dim != 64 && head_dim != 128) return fail(PARO_ERR_INVALID, "paro_attn_prompt: head_dim must be 64 or 128 (got %d)", head_dim);
  if (rows < 1) return fail(PARO_ERR_INVALID, "paro_attn_prompt: rows must be >= 1 (got %lld)", (long long)rows);
  if (pos0 < 0 || max_positions < 1 || max_positions % 8 != 0 || (int64_t)pos0 + rows > (int64_t)max_positions)
    return fail(PARO_ERR_INVALID, "paro_attn_prompt: positions pos0 %d + rows %lld exceed max_positions %d (a positive multiple of 8)", pos0,
                (long long)rows, max_positions);
  if (n_heads < 1 || n_kv_heads < 1 || n_kv_heads > 65535 || n_heads % n_kv_heads != 0 || n_heads / n_kv_heads > kApRows)
    return fail(PARO_ERR_INVALID, "paro_attn_prompt: n_heads %d must be a multiple of n_kv_heads %d, at most %d per KV head", n_heads, n_kv_heads,
                kApRows);
  if (act_dtype != PARO_DTYPE_F16 && act_dtype != PARO_DTYPE_BF16) return fail(PARO_ERR_INVALID, "paro_attn_prompt: act_dtype must be f16 or bf16");
  if (!q || !kcache || !vcache || !out) return fail(PARO_ERR_INVALID, "paro_attn_prompt: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const int R = (int)rows;
  if (act_dtype == PARO_DTYPE_F16) {
    if (head_dim == 64) launch_attn_prompt<f16, 64>(q, kcache, vcache, out, R, pos0, n_heads, n_kv_heads, max_positions, st);
    else launch_attn_prompt<f16, 128>(q, kcache, vcache, out, R, pos0, n_heads, n_kv_heads, max_positions, st);
  } else {
    if (head_dim == 64) launch_attn_prompt<bf16, 64>(q, kcache, vcache, out, R, pos0, n_heads, n_kv_heads, max_positions, st);
    else launch_attn_prompt<bf16, 128>(q, kcache, vcache, out, R, pos0, n_heads, n_kv_heads, max_positions, st);
  }
  return check_launch("paro_attn_prompt");
}
