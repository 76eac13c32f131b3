// Best-of-K sampled decoding: K tours per instance from ONE encoding.
//
// The virtual batch has V = K B elements, element j = k B + b being sample k of instance b.  The
// encoder and the decoder prologue run on the B real instances; everything here reads their
// per-instance tables through b = j % B and keeps the per-element episode state (visited row, the
// two mask buffers, current / last / first node, fp64 load, the two accumulators) in a workspace of
// its own, indexed by j.  Whatever the reference couples across the batch is coupled across the V
// elements: head h of element j adds the mask row of element (8 j + h) mod V (QUIRK D3), and
// `done` is the whole virtual batch's.
//
//   multi_first_table_kernel  SF[b][f][h][n] = SG[b][h][n] + (Wq_first e_f)_h . K_n / sqrt(48):
//                             the first chosen node's part of every later score row (TSP/VRP,
//                             graph_decoder.py:111-113) for EVERY possible first node, so that a
//                             step's row is SL[b][last] + SF[b][first] for any element
//   multi_init_kernel         element state := the instance's start state
//   multi_step_kernel         one decode + env step for all V elements (the table-driven step of
//                             decoder_rt_body.h, tables by b, state by j)
//   multi_select_kernel       per-instance argmax over k, gathers, final env state
#include "decoder_step.h"
#include "x3_common.h"

struct MultiWs {
  float *SF;                   // (B,N,8,N)  TSP/VRP only
  uint8_t *visited;            // (V,N)
  uint8_t *mask;               // (2,V,N)    ping-pong, as vrp_env::mask
  uint8_t *dep_pre;            // (V)        the depot's visited flag BEFORE the last step's fix-ups
  int32_t *cur, *last, *first; // (V)
  double *load;                // (V)
};

static inline size_t multi_sf_floats(int kind, int B, int N) {
  return kind == VRP_KIND_IRP ? 0 : (size_t)B * N * 8 * N;
}

static inline MultiWs carve_multiws(void *ws, int kind, int B, int N, int K) {
  char *p = (char *)ws;
  const size_t V = (size_t)K * B;
  MultiWs w;
  w.SF = (float *)p;        p += vrp_align_up(multi_sf_floats(kind, B, N) * 4);
  w.load = (double *)p;     p += vrp_align_up(V * 8);
  w.cur = (int32_t *)p;     p += vrp_align_up(V * 4);
  w.last = (int32_t *)p;    p += vrp_align_up(V * 4);
  w.first = (int32_t *)p;   p += vrp_align_up(V * 4);
  w.visited = (uint8_t *)p; p += vrp_align_up(V * N);
  w.mask = (uint8_t *)p;    p += vrp_align_up(2 * V * N);
  w.dep_pre = (uint8_t *)p; p += vrp_align_up(V);
  return w;
}

extern "C" int64_t vrp_multi_workspace_bytes(int kind, int B, int N, int K) {
  if (kind < 0 || kind > 2 || B < 1 || N < 1 || K < 1) return 0;
  const size_t V = (size_t)K * B;
  return (int64_t)(vrp_align_up(multi_sf_floats(kind, B, N) * 4) + vrp_align_up(V * 8) +
                   3 * vrp_align_up(V * 4) + vrp_align_up(V * N) + vrp_align_up(2 * V * N) +
                   vrp_align_up(V));
}

// ------------------------------------------------------------------ first-node score table
// Work unit = (G consecutive graphs, head h), four waves.  Two products per graph, both on the
// bf16 matrix cores with every fp32 operand split into three bf16 planes (x3_common.h: six MFMAs
// per product, fp32 accuracy):
//   stage 1  F[f][k] = sum_c AfT[128 h + k][c] e_f[c]        (N x 128, inner 128)
//   stage 2  SF[f][n] = SG[n] + sum_k F[f][k] e_n[k]          (N x N,   inner 128)
// The head's 128 rows of AfT are split once per workgroup and stay in registers (wave w owns
// columns 32 w .. 32 w + 31 of F) while the workgroup walks its G graphs; the embedding rows and
// F live in LDS as fp32 and are split by the lane that loads them.  MFMA operand order: the
// first operand's rows land in a lane's four registers (row 4 q + r), the second's on lane & 15.
// Stage 2 takes the embedding rows n first, so a lane owns four consecutive n of one table row f:
// 16-byte stores when N % 4 == 0.
#define SF_PITCH 132   // floats per LDS row: 128 + 4, rows 16-byte aligned and off the same banks
typedef float mf32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void sf_split_row(const float *src, bf16x8 (&pl)[3]) {
  const float4 a = *reinterpret_cast<const float4 *>(src);
  const float4 b = *reinterpret_cast<const float4 *>(src + 4);
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  x3_split8(x, pl[0], pl[1], pl[2]);
}
// acc += A B^T over one 32-wide k chunk, small terms first (as encoder_x3.h: x3_mma)
__device__ __forceinline__ mf32x4 sf_mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], mf32x4 acc) {
  acc = X3_MFMA(a[1], b[1], acc);
  acc = X3_MFMA(a[2], b[0], acc);
  acc = X3_MFMA(a[0], b[2], acc);
  acc = X3_MFMA(a[1], b[0], acc);
  acc = X3_MFMA(a[0], b[1], acc);
  acc = X3_MFMA(a[0], b[0], acc);
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void multi_first_table_kernel(int B, int N, int G,
                                                                const float *__restrict__ emb,
                                                                const float *__restrict__ AfT,
                                                                const float *__restrict__ SG,
                                                                float *__restrict__ SF) {
  extern __shared__ __attribute__((aligned(16))) float sf_smem[];
  const int NT = (N + 15) >> 4, R = NT * 16;
  float *Es = sf_smem, *Fs = sf_smem + (size_t)R * SF_PITCH;
  const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, q = lane >> 4;
  bf16x8 wf[2][4][3];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      sf_split_row(AfT + (size_t)(h * 128 + 16 * (2 * wave + c) + i16) * 128 + 32 * j + 8 * q,
                   wf[c][j]);
  for (int g = 0; g < G; ++g) {
    const int b = blockIdx.x * G + g;
    if (b >= B) break;   // workgroup-uniform
    __syncthreads();     // the previous graph's stage 2 has read Es / Fs
    for (int i = tid; i < R * 32; i += 256) {
      const int row = i >> 5, c4 = i & 31;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < N) v = reinterpret_cast<const float4 *>(emb + ((size_t)b * N + row) * VRP_EMB)[c4];
      *reinterpret_cast<float4 *>(Es + row * SF_PITCH + 4 * c4) = v;
    }
    __syncthreads();
    for (int rt = 0; rt < NT; ++rt) {
      mf32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x8 e[3];
        sf_split_row(Es + (16 * rt + i16) * SF_PITCH + 32 * j + 8 * q, e);
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[c] = sf_mma6(wf[c][j], e, acc[c]);
      }
      // D[k = 16 (2 wave + c) + 4 q + r][f = 16 rt + i16]
#pragma unroll
      for (int c = 0; c < 2; ++c)
        *reinterpret_cast<float4 *>(Fs + (16 * rt + i16) * SF_PITCH + 16 * (2 * wave + c) + 4 * q) =
            make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    }
    __syncthreads();
    for (int tile = wave; tile < NT * NT; tile += 4) {
      const int nt = tile / NT, ft = tile - nt * NT;
      mf32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x8 a[3], f3[3];
        sf_split_row(Es + (16 * nt + i16) * SF_PITCH + 32 * j + 8 * q, a);
        sf_split_row(Fs + (16 * ft + i16) * SF_PITCH + 32 * j + 8 * q, f3);
        acc = sf_mma6(a, f3, acc);
      }
      // D[n = 16 nt + 4 q + r][f = 16 ft + i16]
      const int f = 16 * ft + i16, n0 = 16 * nt + 4 * q;
      if (f < N && n0 < N) {
        float *out = SF + (((size_t)b * N + f) * 8 + h) * N + n0;
        const float *sg = SG + ((size_t)b * 8 + h) * N + n0;
        if (VEC) {   // N % 4 == 0: n0 + 3 < N, both rows 16-byte aligned
          const float4 s = *reinterpret_cast<const float4 *>(sg);
          *reinterpret_cast<float4 *>(out) =
              make_float4(s.x + acc[0], s.y + acc[1], s.z + acc[2], s.w + acc[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + r < N) out[r] = sg[r] + acc[r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ element state
struct MultiParams {
  int kind, B, N, K, V, t, max_steps;
  const float *row0, *SL, *SLD, *SF, *RT, *cvec;   // per-instance tables (DecWs, MultiWs::SF)
  const double *pos, *demand;                      // per-instance data (vrp_env)
  const int32_t *depot;
  MultiWs st;                                      // per-element state
  float clip;
  vrp_multi_io io;
};

// element j starts where its instance stands after the rollout's set-up kernel (mask buffer 0,
// visited with the depot fix-ups, current_location, load): tsp.py:150-160,172-174
__global__ __launch_bounds__(256) void multi_init_kernel(MultiParams p, vrp_env env) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int N = p.N, B = p.B;
  if (i >= (size_t)p.V * N) return;
  const int j = (int)(i / N), n = (int)(i - (size_t)j * N), b = j % B;
  p.st.visited[i] = env.visited[(size_t)b * N + n];
  p.st.mask[i] = env.mask[(size_t)b * N + n];
  if (n == 0) {
    p.st.cur[j] = env.cur[b];
    p.st.last[j] = 0;
    p.st.first[j] = 0;
    p.st.dep_pre[j] = 0;
    p.st.load[j] = (p.kind == VRP_KIND_IRP) ? env.load[b] : 1.0;
    p.io.all_loss[j] = 0.f;
    p.io.all_logp[j] = 0.f;
  }
}

// ------------------------------------------------------------------ the multi-sample step
// A copy of decoder_rt_body.h's step_rt_body (large-batch instance, sampling only) for one element
// per wave -- a change to the softmax, the sampling or the env step there belongs here too (DESIGN.md
// 10 says why it is a copy).  Wave w of the grid takes sample k = w % K
// of instance b = w / K, so the four waves of a workgroup (and the workgroups next to it) read the
// same instance's row0 / SL / SF / SLD / RT / cvec rows and coordinates: one fetch from memory,
// the rest from the caches.  Masked rows of RT are never read.  The arithmetic is the
// table-driven step's: fp32 scores and logits, fp64 edge length and IRP load.
template <int NPL>
__device__ __forceinline__ void multi_step_body(const MultiParams &p, float (&a_s)[4][8 * 64 * NPL],
                                                float (&u_s)[4][64 * NPL],
                                                int (&sel_s)[4][64 * NPL]) {
  constexpr int WPG = 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = p.N, B = p.B, V = p.V, t = p.t;
  const int wraw = blockIdx.x * WPG + wave;
  const bool active = wraw < V;
  const int w = __builtin_amdgcn_readfirstlane(active ? wraw : V - 1);
  const int b = w / p.K, j = (w - b * p.K) * B + b;
  const int par = t & 1;
  const uint8_t *mask_in = p.st.mask + (size_t)par * V * N;
  uint8_t *mask_out = p.st.mask + (size_t)(par ^ 1) * V * N;
  const int n4 = 2 * N;  // float4 per RT row (8N floats)
  const int rsl = lane >> 3, part = lane & 7;
  bool inN[NPL];
  int ln[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) { inN[i] = lane + 64 * i < N; ln[i] = inN[i] ? lane + 64 * i : 0; }

  // the virtual batch was done before this launch (tsp.py:95); workgroup-uniform
  if (t > 0 && p.io.notdone[t - 1] == 0) return;
  // ---- entry: issue every action-independent load --------------------------------
  const size_t row = (size_t)b * 8 * N;
  const float *srow = p.row0 + row;
  const float *frow = nullptr;   // first-node row (TSP/VRP after step 0)
  if (t > 0) {
    const int last = __builtin_amdgcn_readfirstlane(p.st.last[j]);
    srow = p.SL + ((size_t)b * N + last) * 8 * N;
    if (p.kind != VRP_KIND_IRP) {
      const int first = __builtin_amdgcn_readfirstlane(p.st.first[j]);
      frow = p.SF + ((size_t)b * N + first) * 8 * N;
    }
  }
  int own_mask[NPL];
  float sc[NPL][8], bs[NPL][8], sld[NPL][8], cv[NPL], q_noise[NPL];
  int msk[NPL][8];
  double2 xy[NPL];
  int vis[NPL];
  double dem[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    own_mask[i] = mask_in[(size_t)j * N + ln[i]];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      sc[i][h] = srow[h * N + ln[i]];
      bs[i][h] = frow ? frow[h * N + ln[i]] : 0.f;
      sld[i][h] = (p.kind == VRP_KIND_IRP) ? p.SLD[row + h * N + ln[i]] : 0.f;
      // QUIRK D3 on the virtual batch: element (8 j + h) mod V
      msk[i][h] = mask_in[(size_t)((j * 8 + h) % V) * N + ln[i]];
    }
    cv[i] = p.cvec[(size_t)b * N + ln[i]];
    xy[i] = reinterpret_cast<const double2 *>(p.pos)[(size_t)b * N + ln[i]];
    vis[i] = 1;
    if (inN[i]) vis[i] = p.st.visited[(size_t)j * N + ln[i]];
    dem[i] = 0.0;
    if (p.kind == VRP_KIND_IRP) dem[i] = p.demand[(size_t)b * N + ln[i]];
    q_noise[i] = p.io.noise ? p.io.noise[((size_t)t * V + j) * N + ln[i]]
                            : vrp_exp1_noise(p.io.noise_seed, t, j, ln[i]);
  }
  const int cur = p.st.cur[j];
  const int dep = p.depot[b];
  const double load0 = (p.kind == VRP_KIND_IRP) ? p.st.load[j] : 1.0;
  const float accl = p.io.all_loss[j], accp = p.io.all_logp[j];
  // selectable nodes (own mask == 0); their RT rows are the only ones fetched
  unsigned long long sel[NPL];
  int nsel = 0;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const bool s_i = inN[i] && !own_mask[i];
    sel[i] = __ballot(s_i);
    if (s_i) sel_s[wave][nsel + __popcll(sel[i] & ((1ull << lane) - 1ull))] = lane + 64 * i;
    nsel += __popcll(sel[i]);
  }
  const int cnt = (n4 - part + 7) >> 3;          // float4 of a row owned by this lane
  const int nchunk = (((n4 + 7) >> 3) + RT_U - 1) / RT_U;
  const int total = ((nsel + 7) >> 3) * nchunk;  // work items (pass, chunk), wave-uniform
  const float4 *rtb = reinterpret_cast<const float4 *>(p.RT) + (size_t)b * N * n4 + part;
  constexpr int NB = 2;   // work items in flight: the rows come from the caches
  float4 rbuf[NB][RT_U];
  int mrow[NB];
  int m_first = -1;  // pass 0 rows (k = rsl < 8)
  if (rsl < nsel) {
    const int c0 = __popcll(sel[0]);
    m_first = (NPL == 1 || rsl < c0) ? kth_set_bit(sel[0], rsl)
                                     : 64 + kth_set_bit(sel[NPL - 1], rsl - c0);
  }
  auto load_item = [&](float4 (&r)[RT_U], int wi, int &m_out) {
    const int pass = wi / nchunk, ch = wi - pass * nchunk;
    const int k = 8 * pass + rsl;
    const int m = (pass == 0) ? m_first : (k < nsel ? sel_s[wave][k] : -1);
    m_out = m;
    rt_load(r, rtb + (size_t)(m < 0 ? 0 : m) * n4, ch * RT_U, cnt, m >= 0);
  };
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    mrow[i] = -1;
    if (i < total) load_item(rbuf[i], i, mrow[i]);
  }

  // ---- glimpse attention weights (lane = n): one wave-wide maximum over the eight heads ----
  {
    const float loadf = (float)load0;
    float s[NPL][8], mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPL; ++i)
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        float v = sc[i][h] + bs[i][h];
        if (p.kind == VRP_KIND_IRP) v = fmaf(loadf, sld[i][h], v);
        v = inN[i] ? v + (float)msk[i][h] : -INFINITY;
        s[i][h] = v;
        mx = fmaxf(mx, v);
      }
    const float M = wave_max(mx);
    float e[NPL][8], sum[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      sum[h] = 0.f;
#pragma unroll
      for (int i = 0; i < NPL; ++i) { e[i][h] = inN[i] ? exp_nonpos(s[i][h] - M) : 0.f; sum[h] += e[i][h]; }
    }
    wave_sum8(sum);
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      if (!(sum[h] > 1e-30f)) {  // wave-uniform, practically never: per-head maximum
        float hm = -INFINITY;
#pragma unroll
        for (int i = 0; i < NPL; ++i) hm = fmaxf(hm, s[i][h]);
        hm = wave_max(hm);
        float es = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) { e[i][h] = inN[i] ? exp_nonpos(s[i][h] - hm) : 0.f; es += e[i][h]; }
        sum[h] = wave_sum(es);
      }
      float r = __builtin_amdgcn_rcpf(sum[h]);
      r = fmaf(fmaf(-sum[h], r, 1.f), r, r);
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (inN[i]) a_s[wave][h * N + lane + 64 * i] = e[i][h] * r;
    }
  }
  __syncthreads();

  // ---- u_m = sum_{h,n} a[h][n] * RT[m][h][n] + cvec[m]  for selectable m ---------------
  {
    const float4 *aw = reinterpret_cast<const float4 *>(a_s[wave]) + part;
    float acc = 0.f;
    auto consume = [&](const float4 (&r)[RT_U], int wi, int m) {
      const int ch = wi % nchunk;
      acc = rt_dot(acc, r, aw, ch * RT_U, m >= 0 ? cnt : 0);
      if (ch == nchunk - 1) {
        acc = group8_sum(acc);
        if (part == 0 && m >= 0) u_s[wave][m] = acc;
        acc = 0.f;
      }
    };
    for (int wi = 0; wi < total; wi += NB) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (wi + i < total) {
          consume(rbuf[i], wi + i, mrow[i]);
          if (wi + i + NB < total) load_item(rbuf[i], wi + i + NB, mrow[i]);
        }
      }
    }
  }
  __syncthreads();

  float u[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    u[i] = -INFINITY;
    if (inN[i] && !own_mask[i])
      u[i] = p.clip * tanhf(u_s[wave][lane + 64 * i] + cv[i]);  // graph_decoder.py:97-98
  }

  // lowest node index among the maxima (torch CPU argmax): slot 0 holds nodes < 64
  auto argmax_nodes = [&](const float (&v)[NPL]) {
    float mx = v[0];
#pragma unroll
    for (int i = 1; i < NPL; ++i) mx = fmaxf(mx, v[i]);
    const float m = wave_max(mx);
    int res = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const unsigned long long hit = __ballot(v[i] == m);
      if (!found && hit) { res = 64 * i + __ffsll((long long)hit) - 1; found = true; }
    }
    return res;
  };

  // Categorical(logits=u): logits - logsumexp, probs = softmax, sample = argmax(p/q)
  int idx;
  float logp;
  {
    float mx = u[0];
#pragma unroll
    for (int i = 1; i < NPL; ++i) mx = fmaxf(mx, u[i]);
    const float m = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) se += expf(u[i] - m);
    se = wave_sum(se);
    const float lse = m + logf(se);
    float l[NPL], lmx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { l[i] = u[i] - lse; lmx = fmaxf(lmx, l[i]); }
    const float lm = wave_max(lmx);
    float pe[NPL], ps = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { pe[i] = expf(l[i] - lm); ps += pe[i]; }
    ps = wave_sum(ps);
    float ratio[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) ratio[i] = inN[i] ? (pe[i] / ps) / q_noise[i] : -1.f;
    idx = argmax_nodes(ratio);
    const float lsel = (NPL > 1 && idx >= 64) ? l[NPL - 1] : l[0];
    logp = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lsel),
                                                               idx & 63));
  }
  idx = __builtin_amdgcn_readfirstlane(idx);
  if (!active) return;  // wave-uniform; no barriers below

  // ---- env.step on registers (same operation order as env_device.h) -------------------
  auto node_f64 = [&](const double (&v)[NPL], int n) {
    return (NPL > 1 && n >= 64) ? readlane_f64(v[NPL - 1], n - 64) : readlane_f64(v[0], n);
  };
  double px[NPL], py[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) { px[i] = xy[i].x; py[i] = xy[i].y; }
#pragma unroll
  for (int i = 0; i < NPL; ++i) if (lane + 64 * i == idx) vis[i] = 1;  // tsp.py:86
  const double dx = node_f64(px, cur) - node_f64(px, idx);
  const double dy = node_f64(py, cur) - node_f64(py, idx);
  const double dist = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
  double load = 1.0;
  if (p.kind == VRP_KIND_IRP) {                               // irp.py:80-86
    load = load0 - node_f64(dem, idx);
    if (idx == dep) load = 1.0;
  }
  auto all_visited = [&]() {
    int ok = 1;
#pragma unroll
    for (int i = 0; i < NPL; ++i) ok &= vis[i];
    return __all(ok);
  };
  const bool done = all_visited();                            // before the fix-ups, tsp.py:95
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    if (lane + 64 * i == dep) {
      p.st.dep_pre[j] = (uint8_t)vis[i];                      // what is_done() saw (selection)
      if (idx == dep) vis[i] = 1;                             // tsp.py:141-142
      else if (p.kind != VRP_KIND_TSP) vis[i] = 0;            // vrp.py:28-31
    }
  }
  if (all_visited()) {                                        // tsp.py:145-146
#pragma unroll
    for (int i = 0; i < NPL; ++i) if (lane + 64 * i == dep) vis[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    int mk = vis[i];
    if (p.kind == VRP_KIND_IRP && inN[i] && dem[i] - load > 0.0) mk = 1;  // irp.py:151-153
    if (inN[i]) {
      p.st.visited[(size_t)j * N + lane + 64 * i] = (uint8_t)vis[i];
      mask_out[(size_t)j * N + lane + 64 * i] = (uint8_t)mk;
    }
  }
  if (lane == 0) {
    p.st.cur[j] = idx;
    if (p.kind == VRP_KIND_IRP) p.st.load[j] = load;
    p.io.all_loss[j] = accl + (float)(-dist);  // fp32 accumulate in step order, tsp_agent:85
    p.io.all_logp[j] = accp + logp;
    p.st.last[j] = idx;
    if (t == 0) p.st.first[j] = idx;
    if (!done) p.io.notdone[t] = 1;   // plain store, every writer the same value (decoder_rt_body.h)
    p.io.all_actions[(size_t)t * V + j] = idx;
    if (p.io.step_logp) p.io.step_logp[(size_t)t * V + j] = logp;
  }
}

template <int NPL>  // nodes per lane: 1 (N <= 64) or 2 (N <= 128); node = lane + 64*i
__global__ __launch_bounds__(256, (NPL == 1 ? 3 : 2)) void multi_step_kernel(MultiParams p) {
  constexpr int NMAXL = 64 * NPL;
  __shared__ __attribute__((aligned(16))) float a_s[4][8 * NMAXL];  // a[h][n], hn order
  __shared__ __attribute__((aligned(16))) float u_s[4][NMAXL];
  __shared__ int sel_s[4][NMAXL];  // compacted list of selectable nodes
  multi_step_body<NPL>(p, a_s, u_s, sel_s);
}

// ------------------------------------------------------------------ selection
// One wave per instance: best_k[b] = the lowest k among the largest all_loss[k][b] (the shortest
// tour; two samples that drew the same tour tie exactly), the chosen sample's accumulators and
// actions, and its final state into the env's (B,N) tensors: visited as the last env.step left it
// when it evaluated `done` (tsp.py:95, i.e. before the mask fix-ups of the get_state that
// follows), current_location and load.
__global__ __launch_bounds__(256) void multi_select_kernel(MultiParams p, vrp_env env) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int B = p.B, N = p.N, K = p.K, V = p.V;
  if (b >= B) return;
  float best = -INFINITY;
  int bk = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const float v = p.io.all_loss[(size_t)k * B + b];
    if (v > best || bk == 0x7fffffff) { best = v; bk = k; }   // ascending k: the first maximum stays
  }
  wave_argmax(best, bk);
  bk = __builtin_amdgcn_readfirstlane(bk);
  const int j = bk * B + b;
  for (int t = lane; t < p.max_steps; t += 64)
    p.io.actions[(size_t)t * B + b] = p.io.all_actions[(size_t)t * V + j];
  const int dep = p.depot[b];
  for (int n = lane; n < N; n += 64) {
    uint8_t v = p.st.visited[(size_t)j * N + n];
    if (n == dep) v = p.st.dep_pre[j];
    env.visited[(size_t)b * N + n] = v;
  }
  if (lane == 0) {
    p.io.best_k[b] = bk;
    p.io.acc_loss[b] = p.io.all_loss[j];
    p.io.acc_logp[b] = p.io.all_logp[j];
    env.cur[b] = p.st.cur[j];
    if (p.kind == VRP_KIND_IRP) env.load[b] = p.st.load[j];
  }
}

// ------------------------------------------------------------------ host side
static MultiParams multi_params(int kind, const vrp_env *env, void *dec_workspace,
                                void *multi_workspace, const vrp_multi_io *io, int K,
                                int max_steps) {
  MultiParams p;
  const int B = env->B, N = env->N;
  DecWs w = carve_decws(dec_workspace, B, N);
  p.kind = kind; p.B = B; p.N = N; p.K = K; p.V = K * B; p.t = 0; p.max_steps = max_steps;
  p.st = carve_multiws(multi_workspace, kind, B, N, K);
  p.row0 = w.row0; p.SL = w.SL; p.SLD = w.SLD; p.SF = p.st.SF; p.RT = w.RT; p.cvec = w.cvec;
  p.pos = env->pos; p.demand = env->demand; p.depot = env->depot;
  p.clip = io->logit_clip > 0.f ? io->logit_clip : 10.f;
  p.io = *io;
  return p;
}

int vrp_multi_tables(int kind, const void *derived, int B, int N, const float *emb,
                     void *dec_workspace, void *multi_workspace, int K, hipStream_t st) {
  if (kind == VRP_KIND_IRP) return 0;   // no first-node term (graph_decoder.py:90-91)
  Derived d = carve_derived(const_cast<void *>(derived));
  DecWs w = carve_decws(dec_workspace, B, N);
  MultiWs m = carve_multiws(multi_workspace, kind, B, N, K);
  const int R = ((N + 15) >> 4) * 16;
  const size_t lds = (size_t)2 * R * SF_PITCH * sizeof(float);   // <= 118 KB at N = 100
  const int G = B >= 512 ? 8 : B >= 256 ? 4 : B >= 128 ? 2 : 1;
  const dim3 grid((B + G - 1) / G, 8);
  static VrpAttrOnce once[2];
  const bool vec = (N & 3) == 0;
  if (!once[vec].done()) {
    const hipError_t e = vec ? hipFuncSetAttribute((const void *)multi_first_table_kernel<true>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)
                             : hipFuncSetAttribute((const void *)multi_first_table_kernel<false>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      vrp_set_error("multi_first_table: raising the LDS limit failed: %s", hipGetErrorString(e));
      return 1;
    }
    once[vec].mark();
  }
  if (vec)
    hipLaunchKernelGGL((multi_first_table_kernel<true>), grid, dim3(256), lds, st, B, N, G, emb, d.AfT,
                       w.SG, m.SF);
  else
    hipLaunchKernelGGL((multi_first_table_kernel<false>), grid, dim3(256), lds, st, B, N, G, emb, d.AfT,
                       w.SG, m.SF);
  VRP_CHECK_LAUNCH("multi_first_table");
  return 0;
}

int vrp_multi_init(int kind, const vrp_env *env, void *dec_workspace, void *multi_workspace,
                   const vrp_multi_io *io, int K, int max_steps, hipStream_t st) {
  const MultiParams p = multi_params(kind, env, dec_workspace, multi_workspace, io, K, max_steps);
  const size_t total = (size_t)p.V * p.N;
  hipLaunchKernelGGL(multi_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p,
                     *env);
  VRP_CHECK_LAUNCH("multi_init");
  return 0;
}

int vrp_multi_step(int kind, const vrp_env *env, void *dec_workspace, void *multi_workspace,
                   const vrp_multi_io *io, int K, int t, int max_steps, hipStream_t st) {
  MultiParams p = multi_params(kind, env, dec_workspace, multi_workspace, io, K, max_steps);
  p.t = t;
  const dim3 grid((p.V + 3) / 4);
  if (p.N <= 64) hipLaunchKernelGGL((multi_step_kernel<1>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((multi_step_kernel<2>), grid, dim3(256), 0, st, p);
  VRP_CHECK_LAUNCH("multi_step");
  return 0;
}

int vrp_multi_select(int kind, const vrp_env *env, void *dec_workspace, void *multi_workspace,
                     const vrp_multi_io *io, int K, int max_steps, hipStream_t st) {
  const MultiParams p = multi_params(kind, env, dec_workspace, multi_workspace, io, K, max_steps);
  hipLaunchKernelGGL(multi_select_kernel, dim3((p.B + 3) / 4), dim3(256), 0, st, p, *env);
  VRP_CHECK_LAUNCH("multi_select");
  return 0;
}
