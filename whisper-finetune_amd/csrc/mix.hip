// mix.hip — loudness normalisation (ITU-R BS.1770) and background noise over a ragged batch (include/wft.h "Loudness and background
// noise" is the contract).
//
// wft_loudness_f32: the K-weighting cascade (two biquads, fp64) is cut along time as in filter.hip — chunks of MX_L samples from zero
// state, a per-row scan of the chunk states, the chunks again from their true state — but the second pass keeps no filtered sample:
// a chunk thread adds y^2 into the at most two hop-slots its chunk touches (hop >= MX_L) and writes the two fp64 partials.  One
// workgroup per row then adds the partials of each slot in chunk order, forms the block energies from four consecutive slots, runs
// the two gates and leaves the row's statistics and its f32 gain; the apply pass is the 4-samples-per-thread copy or multiply of
// wavefx.hip.  Launches: local, scan, energy, gate, apply (the last one only with an output).
// wft_bg_mix_f32: two sums of squares per active row (the clip, the noise segment) in the chunked order of wavefx.hip's
// wf_sumsq_kernel, restated here, one thread per row for the scale, then out = f32(x + scale * s).  Launches: sumsq, scale, mix.
// The statistic launches are fixed grids looping over (row, chunk) items; an item of a row that is not active ends at once, so their
// cost follows the active rows.  No float atomics; every sum has a fixed order that does not depend on B or the launch.
// Side kernels of the loader: plain C++, nothing hand-scheduled.  The fp64 arithmetic is the contract, so contraction is off.
#include "common.h"

#pragma clang fp contract(off)

#define MX_L 512                      // samples per chunk of the K-weighting passes
#define MX_G 64                       // chunks per workgroup = threads per workgroup (one wave)
#define MX_P 32                       // samples of every chunk staged per piece
#define MX_LDP (MX_P + 1)
#define MX_T 256                      // threads per workgroup of the other kernels
#define MX_TILE (4 * MX_T)
#define MX_TRIPS 4
#define MX_SPAN (MX_TILE * MX_TRIPS)  // samples per workgroup of an apply pass
#define MX_CHUNK 4096                 // samples per item of bg_mix's sums
#define MX_GRID 1024                  // workgroups of bg_mix's sum launch
#define MX_MAX_N (1 << 30)
#define MX_HOP_MAX (1 << 24)

struct mx_sos { double c[2][5]; };    // b0 b1 b2 a1 a2 of the two sections, by value

__device__ __forceinline__ int mx_row_len(const int* n, int b, int n_max) { return n ? min(max(n[b], 0), n_max) : n_max; }

// one sample through the two sections: direct form II transposed, as scipy.signal.lfilter does it
__device__ __forceinline__ double mx_step(const mx_sos& k, double (&z)[2][2], double x) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double y = k.c[s][0] * x + z[s][0];
    z[s][0] = k.c[s][1] * x - k.c[s][3] * y + z[s][1];
    z[s][1] = k.c[s][2] * x - k.c[s][4] * y;
    x = y;
  }
  return x;
}

// ------------------------------------------------------------------------------------------------------------ 4-sample access
__device__ __forceinline__ void mx_load4(const float* row, bool vec, int i, int n_b, float (&v)[4]) {
  if (vec && i + 4 <= n_b) {
    const float4 q = *reinterpret_cast<const float4*>(row + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n_b ? row[i + k] : 0.f;
  }
}
__device__ __forceinline__ void mx_store4(float* row, bool vec, int i, int hi, const float (&v)[4]) {
  if (vec && i + 4 <= hi) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < hi) row[i + k] = v[k];
  }
}
__device__ __forceinline__ bool mx_vec_ok(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------ loudness: chunks
// piece p of the workgroup's MX_G chunks -> registers: element e = lane + 64 k is sample (e % MX_P) of chunk e / MX_P
__device__ __forceinline__ void mx_load_piece(const float* row, int base, int p, int n_b, int lane, float (&v)[MX_P]) {
#pragma unroll
  for (int k = 0; k < MX_P; ++k) {
    const int e = lane + MX_G * k;
    const int i = base + (e / MX_P) * MX_L + p * MX_P + (e % MX_P);
    v[k] = i < n_b ? row[i] : 0.f;
  }
}
__device__ __forceinline__ void mx_piece_to_lds(float* lds, int lane, const float (&v)[MX_P]) {
#pragma unroll
  for (int k = 0; k < MX_P; ++k) {
    const int e = lane + MX_G * k;
    lds[(e / MX_P) * MX_LDP + (e % MX_P)] = v[k];
  }
}

// a row is measured when the call measures only (no output) or the row is normalised
__device__ __forceinline__ bool mx_measured(const int* mode, int b, int measure_all) { return measure_all || (mode && mode[b] == 1); }

// ENERGY false: every chunk from zero state, its final state -> state[b][c][4].  ENERGY true: every chunk from its true state
// (state[b][c], after the scan); sum of y^2 over the chunk's samples in front of the first hop boundary inside it -> part[b][c][0],
// behind it -> part[b][c][1], each in ascending sample order.
template <bool ENERGY>
__global__ __launch_bounds__(MX_G) void mx_chunk_kernel(const float* in, long ld_in, const int* n, int n_max, mx_sos k, int hop,
                                                        const int* mode, int measure_all, double* state, double* part, int C) {
  __shared__ float lds[MX_G * MX_LDP];
  const int lane = threadIdx.x, b = blockIdx.y, base = blockIdx.x * (MX_G * MX_L);
  const int n_b = mx_row_len(n, b, n_max);
  if (base >= n_b || n_b < 4 * hop || !mx_measured(mode, b, measure_all)) return;  // uniform over the workgroup
  const float* row = in + b * ld_in;
  const int start = base + lane * MX_L;
  const int len = min(max(n_b - start, 0), MX_L);  // samples of this thread's chunk
  const int ch = blockIdx.x * MX_G + lane;
  double z[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  if (ENERGY && ch < C && len > 0) {
    const double* w = state + ((long)b * C + ch) * 4;
    z[0][0] = w[0]; z[0][1] = w[1]; z[1][0] = w[2]; z[1][1] = w[3];
  }
  const int cut = (start / hop + 1) * hop - start;  // samples of the chunk in its first slot (>= 1; >= MX_L: the chunk has one slot)
  double e0 = 0.0, e1 = 0.0;
  float pre[MX_P];
  mx_load_piece(row, base, 0, n_b, lane, pre);
#pragma unroll 1
  for (int p = 0; p < MX_L / MX_P; ++p) {
    mx_piece_to_lds(lds, lane, pre);
    __syncthreads();
    if (p + 1 < MX_L / MX_P) mx_load_piece(row, base, p + 1, n_b, lane, pre);
#pragma unroll 4
    for (int j = 0; j < MX_P; ++j) {
      const int q = p * MX_P + j;
      if (q < len) {
        const double y = mx_step(k, z, (double)lds[lane * MX_LDP + j]);
        if (ENERGY) {
          if (q < cut) e0 += y * y;
          else e1 += y * y;
        }
      }
    }
    __syncthreads();
  }
  if (ch < C && len > 0) {
    if (ENERGY) {
      double* w = part + ((long)b * C + ch) * 2;
      w[0] = e0; w[1] = e1;
    } else {
      double* w = state + ((long)b * C + ch) * 4;
      w[0] = z[0][0]; w[1] = z[0][1]; w[2] = z[1][0]; w[3] = z[1][1];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ loudness: scan
__device__ __forceinline__ double mx_readlane(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

// one wave per row: column j of the MX_L-step zero-input transition matrix M from the unit state e_j (the same step function), then
// s_0 = 0, s_(c+1) = M s_c + z_c (products in ascending column order, then z_c) replaces z_c by s_c in place
__global__ __launch_bounds__(64) void mx_scan_kernel(const int* n, int n_max, mx_sos k, int hop, const int* mode, int measure_all,
                                                     double* state, int C) {
  __shared__ double Msh[4][4];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int n_b = mx_row_len(n, b, n_max);
  const int nc = (n_b + MX_L - 1) / MX_L;
  if (n_b < 4 * hop || !mx_measured(mode, b, measure_all)) return;  // uniform
  if (lane < 4) {
    double z[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) { z[s][0] = lane == 2 * s ? 1.0 : 0.0; z[s][1] = lane == 2 * s + 1 ? 1.0 : 0.0; }
#pragma unroll 1
    for (int i = 0; i < MX_L; ++i) mx_step(k, z, 0.0);
#pragma unroll
    for (int s = 0; s < 2; ++s) { Msh[2 * s][lane] = z[s][0]; Msh[2 * s + 1][lane] = z[s][1]; }
  }
  __syncthreads();
  const bool live = lane < 4;
  double m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = live ? Msh[lane][j] : 0.0;
  double* w = state + (long)b * C * 4 + (live ? lane : 0);
  double s = 0.0;
  for (int c0 = 0; c0 < nc; c0 += 8) {
    double zz[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) zz[u] = (live && c0 + u < nc) ? w[(long)(c0 + u) * 4] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (c0 + u < nc) {  // uniform
        if (live) w[(long)(c0 + u) * 4] = s;
        double acc = m[0] * mx_readlane(s, 0);
#pragma unroll
        for (int j = 1; j < 4; ++j) acc += m[j] * mx_readlane(s, j);
        s = acc + zz[u];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ loudness: gate
// thread t's value and count, reduced over the workgroup by halving (s[t] += s[t + h], h = 128 .. 1); every thread gets the totals
__device__ __forceinline__ void mx_reduce(double* sd, int* si, int tid, double& v, int& c) {
  sd[tid] = v; si[tid] = c;
  __syncthreads();
  for (int h = MX_T / 2; h >= 1; h >>= 1) {
    if (tid < h) { sd[tid] += sd[tid + h]; si[tid] += si[tid + h]; }
    __syncthreads();
  }
  v = sd[0]; c = si[0];
  __syncthreads();
}

// the energy of block j: its slots in ascending order (a slot at or behind ns does not exist: the cut last block), over 4 * hop
__device__ __forceinline__ double mx_block_z(const double* slot, int j, int ns, double block) {
  double e = slot[j];
#pragma unroll
  for (int u = 1; u < 4; ++u)
    if (j + u < ns) e += slot[j + u];
  return e / block;
}

// one workgroup per row: slot sums, block energies, both gates -> stats[b] = (L, gamma_r, blocks over both gates, gain), the f32
// gain and whether the row is normalised -> gain[b], flag[b]
__global__ __launch_bounds__(MX_T) void mx_gate_kernel(const int* n, int n_max, int hop, const double* target, const int* mode,
                                                       int measure_all, const double* part, double* slots, int C, int NS, double* stats,
                                                       float* gain, int* flag) {
  __shared__ double sd[MX_T];
  __shared__ int si[MX_T];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n_b = mx_row_len(n, b, n_max);
  const int block = 4 * hop;
  const double ninf = -__longlong_as_double(0x7FF0000000000000LL);
  double L = ninf, gamma = ninf;
  int over = 0;
  const bool measured = mx_measured(mode, b, measure_all);
  if (measured && n_b >= block) {  // uniform
    const int ns = (n_b + hop - 1) / hop;
    const int q = (n_b - block) / hop, r = (n_b - block) % hop;
    const int nb = q + 1 + ((2 * (long)r > hop || (2 * (long)r == hop && (q & 1))) ? 1 : 0);  // int(np.round((T - 0.4) / 0.1)) + 1
    const double* pr = part + (long)b * C * 2;
    double* slot = slots + (long)b * NS;
    for (int k = tid; k < ns; k += MX_T) {  // the partials of slot k in chunk order
      const long lo = (long)k * hop, hi = min(lo + hop, (long)n_b);
      double e = 0.0;
      for (int c = (int)(lo / MX_L); c <= (int)((hi - 1) / MX_L); ++c) {
        const int first = (int)(((long)c * MX_L) / hop);  // the slot of the chunk's first sample
        e += pr[2 * c + (first == k ? 0 : 1)];
      }
      slot[k] = e;
    }
    __syncthreads();
    double sum = 0.0;
    int cnt = 0;
    for (int j = tid; j < nb; j += MX_T) {
      const double z = mx_block_z(slot, j, ns, (double)block);
      const double l = -0.691 + 10.0 * log10(z);
      if (l >= -70.0) { sum += z; ++cnt; }
    }
    mx_reduce(sd, si, tid, sum, cnt);
    if (cnt > 0) {  // uniform
      gamma = -0.691 + 10.0 * log10(sum / (double)cnt) - 10.0;
      sum = 0.0; cnt = 0;
      for (int j = tid; j < nb; j += MX_T) {
        const double z = mx_block_z(slot, j, ns, (double)block);
        const double l = -0.691 + 10.0 * log10(z);
        if (l > gamma && l > -70.0) { sum += z; ++cnt; }
      }
      mx_reduce(sd, si, tid, sum, cnt);
      if (cnt > 0) { L = -0.691 + 10.0 * log10(sum / (double)cnt); over = cnt; }
    }
  }
  if (tid == 0) {
    float g = 1.0f;
    int on = 0;
    if (measured && mode && mode[b] == 1 && target && over > 0 && isfinite(L) && isfinite(target[b])) {
      g = (float)exp10((target[b] - L) / 20.0);
      on = 1;
    }
    stats[4 * b] = L; stats[4 * b + 1] = gamma; stats[4 * b + 2] = (double)over; stats[4 * b + 3] = (double)g;
    gain[b] = g; flag[b] = on;
  }
}

__global__ __launch_bounds__(MX_T) void mx_gain_kernel(const float* in, long ld_in, const int* n, int n_max, const float* gain,
                                                       const int* flag, float* out, long ld_out, int inplace) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n_b = mx_row_len(n, b, n_max);
  const bool active = flag[b] != 0;
  if (inplace && !active) return;  // uniform
  const int hi = inplace ? n_b : n_max;
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const bool vin = mx_vec_ok(row), vout = mx_vec_ok(orow);
  const float g = gain[b];
#pragma unroll 1
  for (int t = 0; t < MX_TRIPS; ++t) {
    const int i = blockIdx.x * MX_SPAN + t * MX_TILE + 4 * tid;
    if (i >= hi) break;
    float v[4];
    mx_load4(row, vin, i, n_b, v);
    if (active) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < n_b) v[k] = v[k] * g;
    }
    mx_store4(orow, vout, i, hi, v);
  }
}

// ------------------------------------------------------------------------------------------------------------ background noise
// the entry of row b: its first sample, its length m (0: no usable entry) and the offset, clamped into the entry
__device__ __forceinline__ const float* mx_entry(const wft_bg_rec& r, const float* bank, const long long* bank_off, int K, long long& m,
                                                 long long& off) {
  const int e = min(max(r.entry, 0), K - 1);
  const long long a = bank_off[e];
  m = max(bank_off[e + 1] - a, 0LL);
  off = m > 0 ? min(max((long long)r.offset, 0LL), m - 1) : 0;
  return bank + a;
}
__device__ __forceinline__ bool mx_bg_kind(int kind) { return kind == WFT_BG_SNR || kind == WFT_BG_ABSOLUTE; }

// item (row, which, chunk): which 0 = the clip's n[b] samples, 1 = the first min(m, n[b]) samples of the noise segment.  The order is
// wf_sumsq_kernel's: thread t adds its samples base + t, base + t + 256, ... ascending, the 256 sums are halved pairwise.
__global__ __launch_bounds__(MX_T) void mx_sumsq_kernel(const float* in, long ld_in, const int* n, int n_max, const float* bank,
                                                        const long long* bank_off, int K, const wft_bg_rec* rec, double* partial, int C,
                                                        int B) {
  __shared__ double s[MX_T];
  const int tid = threadIdx.x;
  const long items = (long)B * 2 * C;
  for (long w = blockIdx.x; w < items; w += gridDim.x) {
    const int b = (int)(w / (2 * C)), which = (int)((w / C) & 1), c = (int)(w % C);
    if (!mx_bg_kind(rec[b].kind)) {  // uniform: skip the row's remaining items
      w += (2 * C - 1 - (w % (2 * C))) / gridDim.x * gridDim.x;
      continue;
    }
    const int n_b = mx_row_len(n, b, n_max), base = c * MX_CHUNK;
    const float* src = in + b * ld_in;
    long long m = 0, off = 0;
    int cnt = n_b;
    if (which) {
      src = mx_entry(rec[b], bank, bank_off, K, m, off);
      cnt = (int)min((long long)n_b, m);
      src += m > (long long)n_b ? min(off, m - n_b) : 0;  // a long entry does not wrap; a short one starts at 0
    }
    if (base >= cnt) continue;  // uniform
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < MX_CHUNK / MX_T; ++k) {
      const int i = base + k * MX_T + tid;
      if (i < cnt) {
        const double v = (double)src[i];
        acc += v * v;
      }
    }
    s[tid] = acc;
    __syncthreads();
    for (int h = MX_T / 2; h >= 1; h >>= 1) {
      if (tid < h) s[tid] += s[tid + h];
      __syncthreads();
    }
    if (tid == 0) partial[((long)b * 2 + which) * C + c] = s[0];
    __syncthreads();
  }
}

// one thread per row: the chunks' sums in ascending order, both RMS values, the scale -> stats[b] = (clean RMS, noise RMS, scale);
// scale[b] = 0 means "copy the row"
__global__ __launch_bounds__(MX_T) void mx_scale_kernel(const int* n, int n_max, const long long* bank_off, int K, const wft_bg_rec* rec,
                                                        const double* partial, int C, double* scale, double* stats, int B) {
  const int b = blockIdx.x * MX_T + threadIdx.x;
  if (b >= B) return;
  double clean = 0.0, noise = 0.0, sc = 0.0;
  const int kind = rec[b].kind;
  const int n_b = mx_row_len(n, b, n_max);
  if (mx_bg_kind(kind) && n_b > 0) {
    const int e = min(max(rec[b].entry, 0), K - 1);
    const long long m = max(bank_off[e + 1] - bank_off[e], 0LL);
    const int cnt = (int)min((long long)n_b, m);
    double sx = 0.0, sn = 0.0;
    for (int c = 0; c < (n_b + MX_CHUNK - 1) / MX_CHUNK; ++c) sx += partial[((long)b * 2) * C + c];
    for (int c = 0; c < (cnt + MX_CHUNK - 1) / MX_CHUNK; ++c) sn += partial[((long)b * 2 + 1) * C + c];
    clean = sqrt(sx / (double)n_b);
    noise = cnt > 0 ? sqrt(sn / (double)cnt) : 0.0;
    if (noise >= 1e-9 && isfinite(rec[b].db)) {
      const double desired = kind == WFT_BG_SNR ? clean / exp10(rec[b].db / 20.0) : exp10(rec[b].db / 20.0);
      sc = desired / noise;
      if (!isfinite(sc)) sc = 0.0;
    }
  }
  scale[b] = sc;
  stats[3 * b] = clean; stats[3 * b + 1] = noise; stats[3 * b + 2] = sc;
}

__global__ __launch_bounds__(MX_T) void mx_mix_kernel(const float* in, long ld_in, const int* n, int n_max, const float* bank,
                                                      const long long* bank_off, int K, const wft_bg_rec* rec, const double* scale,
                                                      float* out, long ld_out, int inplace) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n_b = mx_row_len(n, b, n_max);
  const double sc = scale[b];
  const bool active = sc != 0.0;
  if (inplace && !active) return;  // uniform
  const int hi = inplace ? n_b : n_max;
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const bool vin = mx_vec_ok(row), vout = mx_vec_ok(orow);
  long long m = 1, off = 0;
  const float* ent = bank;
  if (active) {
    ent = mx_entry(rec[b], bank, bank_off, K, m, off);  // (m >= 1: the noise RMS is not zero)
    off = m > (long long)n_b ? min(off, m - n_b) : 0;
  }
#pragma unroll 1
  for (int t = 0; t < MX_TRIPS; ++t) {
    const int i = blockIdx.x * MX_SPAN + t * MX_TILE + 4 * tid;
    if (i >= hi) break;
    float v[4];
    mx_load4(row, vin, i, n_b, v);
    if (active && i < n_b) {
      long long j = (off + i) % m;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i + k < n_b) v[k] = (float)((double)v[k] + sc * (double)ent[j]);
        if (++j == m) j = 0;
      }
    }
    mx_store4(orow, vout, i, hi, v);
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static inline int64_t mx_round8(int64_t v) { return (v + 7) / 8 * 8; }

static bool mx_overlap_ok(const float* in, int64_t ld_in, const float* out, int64_t ld_out, int64_t n_max, int B) {
  if (in == out && ld_in == ld_out) return true;  // in place is the same pointer and the same stride; anything else must not overlap
  const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (B - 1) * ld_in + n_max);
  const uintptr_t o0 = (uintptr_t)out, o1 = (uintptr_t)(out + (B - 1) * ld_out + n_max);
  return i1 <= o0 || o1 <= i0;
}

// states f64 [B, C, 4] | partials f64 [B, C, 2] | slots f64 [B, NS] | gain f32 [B] | flag i32 [B]
extern "C" int64_t wft_loudness_workspace_bytes(int B, int64_t n_max, int hop) {
  if (B < 1 || B > 65535 || n_max < 1 || n_max > MX_MAX_N || hop < MX_L || hop > MX_HOP_MAX) return -1;
  const int64_t C = cdiv64(n_max, MX_L), NS = cdiv64(n_max, hop);
  return (int64_t)B * (C * 6 + NS) * (int64_t)sizeof(double) + 2 * mx_round8(4 * (int64_t)B);
}

extern "C" int wft_loudness_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* sos, int hop,
                                const double* target, const int32_t* mode, float* out, int64_t ld_out, double* stats, void* workspace,
                                int64_t workspace_bytes, int B, void* stream) {
  WFT_CHECK_ARG(in && sos && stats && workspace, "null pointer");
  WFT_CHECK_ARG(!out || (target && mode), "an output needs target and mode");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= MX_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(hop >= MX_L && hop <= MX_HOP_MAX, "hop outside [512, 2^24]");
  WFT_CHECK_ARG(ld_in >= n_max && (!out || ld_out >= n_max), "leading dimension smaller than the row");
  WFT_CHECK_ARG(workspace_bytes >= wft_loudness_workspace_bytes(B, n_max, hop), "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)mode % 4 == 0 &&
                    (uintptr_t)sos % 8 == 0 && (uintptr_t)target % 8 == 0 && (uintptr_t)stats % 8 == 0 && (uintptr_t)workspace % 8 == 0,
                "in / out / n / mode must be 4-byte, sos / target / stats / workspace 8-byte aligned");
  mx_sos k;
  for (int s = 0; s < 2; ++s) {  // sos is HOST memory: b0 b1 b2 a0 a1 a2 per section
    bool finite = true;
    for (int j = 0; j < 6; ++j) finite = finite && std::isfinite(sos[6 * s + j]);
    WFT_CHECK_ARG(finite && sos[6 * s + 3] == 1.0, "a section must be finite and normalised to a0 == 1");
    k.c[s][0] = sos[6 * s]; k.c[s][1] = sos[6 * s + 1]; k.c[s][2] = sos[6 * s + 2]; k.c[s][3] = sos[6 * s + 4]; k.c[s][4] = sos[6 * s + 5];
  }
  const bool inplace = out && in == out && ld_in == ld_out;
  WFT_CHECK_ARG(!out || mx_overlap_ok(in, ld_in, out, ld_out, n_max, B), "in and out overlap partially");
  hipStream_t st = (hipStream_t)stream;
  const int nm = (int)n_max, C = (int)cdiv64(n_max, MX_L), NS = (int)cdiv64(n_max, hop), groups = (int)cdiv64(n_max, (int64_t)MX_G * MX_L);
  const int all = out ? 0 : 1;
  double* state = (double*)workspace;
  double* part = state + (int64_t)B * C * 4;
  double* slots = part + (int64_t)B * C * 2;
  float* gain = (float*)(slots + (int64_t)B * NS);
  int* flag = (int*)((char*)gain + mx_round8(4 * (int64_t)B));
  hipLaunchKernelGGL(mx_chunk_kernel<false>, dim3(groups, B), dim3(MX_G), 0, st, in, (long)ld_in, n, nm, k, hop, mode, all, state, part, C);
  hipLaunchKernelGGL(mx_scan_kernel, dim3(B), dim3(64), 0, st, n, nm, k, hop, mode, all, state, C);
  hipLaunchKernelGGL(mx_chunk_kernel<true>, dim3(groups, B), dim3(MX_G), 0, st, in, (long)ld_in, n, nm, k, hop, mode, all, state, part, C);
  hipLaunchKernelGGL(mx_gate_kernel, dim3(B), dim3(MX_T), 0, st, n, nm, hop, target, mode, all, (const double*)part, slots, C, NS, stats,
                     gain, flag);
  if (out)
    hipLaunchKernelGGL(mx_gain_kernel, dim3((unsigned)cdiv64(n_max, MX_SPAN), (unsigned)B), dim3(MX_T), 0, st, in, (long)ld_in, n, nm,
                       (const float*)gain, (const int*)flag, out, (long)ld_out, (int)inplace);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// partials f64 [B, 2, ceil(n_max / 4096)] | scale f64 [B]
extern "C" int64_t wft_bg_mix_workspace_bytes(int B, int64_t n_max) {
  if (B < 1 || B > 65535 || n_max < 1 || n_max > MX_MAX_N) return -1;
  return (int64_t)B * (2 * cdiv64(n_max, MX_CHUNK) + 1) * (int64_t)sizeof(double);
}

extern "C" int wft_bg_mix_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const float* bank, const int64_t* bank_off,
                              int K, const wft_bg_rec* rec, float* out, int64_t ld_out, double* stats, void* workspace,
                              int64_t workspace_bytes, int B, void* stream) {
  WFT_CHECK_ARG(in && bank && bank_off && rec && out && stats && workspace, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= MX_MAX_N && K >= 1, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535, K >= 1)");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG(workspace_bytes >= wft_bg_mix_workspace_bytes(B, n_max), "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)bank % 4 == 0 &&
                    (uintptr_t)bank_off % 8 == 0 && (uintptr_t)rec % 8 == 0 && (uintptr_t)stats % 8 == 0 && (uintptr_t)workspace % 8 == 0,
                "in / out / n / bank must be 4-byte, bank_off / rec / stats / workspace 8-byte aligned");
  WFT_CHECK_ARG(mx_overlap_ok(in, ld_in, out, ld_out, n_max, B), "in and out overlap partially");
  const bool inplace = in == out && ld_in == ld_out;
  hipStream_t st = (hipStream_t)stream;
  const int nm = (int)n_max, C = (int)cdiv64(n_max, MX_CHUNK);
  double* partial = (double*)workspace;
  double* scale = partial + (int64_t)B * 2 * C;
  const long long* off = (const long long*)bank_off;
  hipLaunchKernelGGL(mx_sumsq_kernel, dim3(MX_GRID), dim3(MX_T), 0, st, in, (long)ld_in, n, nm, bank, off, K, rec, partial, C, B);
  hipLaunchKernelGGL(mx_scale_kernel, dim3((unsigned)cdiv64(B, MX_T)), dim3(MX_T), 0, st, n, nm, off, K, rec, (const double*)partial, C,
                     scale, stats, B);
  hipLaunchKernelGGL(mx_mix_kernel, dim3((unsigned)cdiv64(n_max, MX_SPAN), (unsigned)B), dim3(MX_T), 0, st, in, (long)ld_in, n, nm, bank, off,
                     K, rec, (const double*)scale, out, (long)ld_out, (int)inplace);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
