// filter.hip — filter augmentation: a batched cascade of second-order sections (include/wft.h "IIR filter").
//
// A row is one sequential recurrence of n samples; a batch of 32..96 rows offers no parallelism unless the recurrence is cut along
// time.  The cascade is ONE linear system with 2 S states, so a row is cut into chunks of SF_L samples and run in three launches:
//   local   one thread per chunk runs the chunk from ZERO state and keeps the state it ends in, z_c            -> ws[b][c][2 S]
//   scan    one wave per row.  Lane j < 2 S runs SF_L zero-input steps of the SAME step function from the unit state e_j: column j of
//           the SF_L-step transition matrix M (it cannot disagree with the recurrence).  Then the sequential scan
//           s_0 = 0, s_(c+1) = M s_c + z_c, lane i holding component i and row i of M, replaces z_c by s_c in place  -> ws[b][c][2 S]
//   apply   one thread per chunk runs the chunk again from its true initial state s_c and writes the outputs, zeros behind n[b].
// Exact in exact arithmetic; in fp64 the reordering costs at most 1.1e-10 of the row's largest output at the extremes of the default
// filter ranges, 5e-13 for all but the widest band-stop (DESIGN.md §3 "Filter augmentation" has the figures).  A workgroup is ONE wave that owns SF_G consecutive chunks.  A thread walking its own chunk would
// read with a stride of SF_L floats between lanes, so the chunks are staged through LDS in pieces of SF_P samples: a piece is loaded
// with 32 neighbouring lanes on 128 contiguous bytes, stored with a row stride of SF_P + 1 floats (a lane's walk along its row and the
// 32 lanes of one load both touch 32 different banks), and the next piece's loads are in flight while the current one is computed.
// The outputs go back the same way.  An in-place call is safe: a workgroup reads and writes only its own SF_G * SF_L samples, a piece
// is loaded before it is stored, and `local` has read the whole row before `apply` starts (stream order).
// Side kernel of the loader (12 bytes per sample): plain C++, nothing hand-scheduled.
#include "common.h"

#define SF_L 512      // samples per chunk
#define SF_G 64       // chunks per workgroup = threads per workgroup (one wave)
#define SF_P 32       // samples of every chunk staged per piece
#define SF_LDP (SF_P + 1)
#define SF_MAX_S 4
#define SF_MAX_N (1 << 30)

// one sample through the cascade: direct form II transposed per section, as scipy.signal.sosfilt does it.  c[s] = b0 b1 b2 a1 a2
template <int S>
__device__ __forceinline__ double sf_step(const double (&c)[S][5], double (&z)[S][2], double x) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const double y = c[s][0] * x + z[s][0];
    z[s][0] = c[s][1] * x - c[s][3] * y + z[s][1];
    z[s][1] = c[s][2] * x - c[s][4] * y;
    x = y;
  }
  return x;
}

// the row's coefficients (wave-uniform loads); returns whether every section is exactly b = 1 0 0, a = . 0 0
template <int S>
__device__ __forceinline__ bool sf_coeffs(const double* sos, int b, double (&c)[S][5]) {
  const double* p = sos + (long)b * S * 6;
  bool ident = true;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    c[s][0] = p[s * 6 + 0]; c[s][1] = p[s * 6 + 1]; c[s][2] = p[s * 6 + 2];
    c[s][3] = p[s * 6 + 4]; c[s][4] = p[s * 6 + 5];
    ident = ident && c[s][0] == 1.0 && c[s][1] == 0.0 && c[s][2] == 0.0 && c[s][3] == 0.0 && c[s][4] == 0.0;
  }
  return ident;
}

__device__ __forceinline__ int sf_row_len(const int* n, int b, int n_max) { return n ? min(max(n[b], 0), n_max) : n_max; }

// piece p of the workgroup's SF_G chunks -> registers: element e = lane + 64 k is sample (e % SF_P) of chunk e / SF_P
__device__ __forceinline__ void sf_load_piece(const float* row, int base, int p, int n_b, int lane, float (&v)[SF_P]) {
#pragma unroll
  for (int k = 0; k < SF_P; ++k) {
    const int e = lane + SF_G * k;
    const int i = base + (e / SF_P) * SF_L + p * SF_P + (e % SF_P);
    v[k] = i < n_b ? row[i] : 0.f;
  }
}
__device__ __forceinline__ void sf_piece_to_lds(float* lds, int lane, const float (&v)[SF_P]) {
#pragma unroll
  for (int k = 0; k < SF_P; ++k) {
    const int e = lane + SF_G * k;
    lds[(e / SF_P) * SF_LDP + (e % SF_P)] = v[k];
  }
}

// ------------------------------------------------------------------------------------------------------------ local
template <int S>
__global__ __launch_bounds__(SF_G) void sos_local_kernel(const float* in, long ld_in, const int* n, int n_max, const double* sos,
                                                         double* ws, int C) {
  __shared__ float lds[SF_G * SF_LDP];
  const int lane = threadIdx.x, b = blockIdx.y, base = blockIdx.x * (SF_G * SF_L);
  const int n_b = sf_row_len(n, b, n_max);
  double c[S][5];
  if (base >= n_b || sf_coeffs<S>(sos, b, c)) return;  // uniform over the workgroup
  const float* row = in + b * ld_in;
  const int len = min(max(n_b - (base + lane * SF_L), 0), SF_L);  // samples of this thread's chunk
  double z[S][2];
#pragma unroll
  for (int s = 0; s < S; ++s) z[s][0] = z[s][1] = 0.0;
  float pre[SF_P];
  sf_load_piece(row, base, 0, n_b, lane, pre);
#pragma unroll 1
  for (int p = 0; p < SF_L / SF_P; ++p) {
    sf_piece_to_lds(lds, lane, pre);
    __syncthreads();
    if (p + 1 < SF_L / SF_P) sf_load_piece(row, base, p + 1, n_b, lane, pre);
#pragma unroll 4
    for (int j = 0; j < SF_P; ++j)
      if (p * SF_P + j < len) sf_step<S>(c, z, (double)lds[lane * SF_LDP + j]);
    __syncthreads();
  }
  const int ch = blockIdx.x * SF_G + lane;
  if (ch < C && len > 0) {
    double* w = ws + ((long)b * C + ch) * (2 * S);
#pragma unroll
    for (int s = 0; s < S; ++s) { w[2 * s] = z[s][0]; w[2 * s + 1] = z[s][1]; }
  }
}

// ------------------------------------------------------------------------------------------------------------ scan
__device__ __forceinline__ double sf_readlane(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

template <int S>
__global__ __launch_bounds__(64) void sos_scan_kernel(const int* n, int n_max, const double* sos, double* ws, int C) {
  constexpr int NS = 2 * S;
  __shared__ double Msh[NS][NS];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int n_b = sf_row_len(n, b, n_max);
  const int nc = (n_b + SF_L - 1) / SF_L;
  double c[S][5];
  if (sf_coeffs<S>(sos, b, c) || nc == 0) return;
  if (lane < NS) {  // column `lane` of M: SF_L zero-input steps from the unit state
    double z[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) { z[s][0] = lane == 2 * s ? 1.0 : 0.0; z[s][1] = lane == 2 * s + 1 ? 1.0 : 0.0; }
#pragma unroll 1
    for (int i = 0; i < SF_L; ++i) sf_step<S>(c, z, 0.0);
#pragma unroll
    for (int s = 0; s < S; ++s) { Msh[2 * s][lane] = z[s][0]; Msh[2 * s + 1][lane] = z[s][1]; }
  }
  __syncthreads();
  const bool live = lane < NS;
  double m[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) m[k] = live ? Msh[lane][k] : 0.0;
  double* w = ws + (long)b * C * NS + (live ? lane : 0);
  double s = 0.0;
  for (int c0 = 0; c0 < nc; c0 += 8) {
    double zz[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) zz[u] = (live && c0 + u < nc) ? w[(long)(c0 + u) * NS] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (c0 + u < nc) {  // uniform
        if (live) w[(long)(c0 + u) * NS] = s;
        double acc = m[0] * sf_readlane(s, 0);
#pragma unroll
        for (int k = 1; k < NS; ++k) acc += m[k] * sf_readlane(s, k);
        s = acc + zz[u];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ apply
template <int S>
__global__ __launch_bounds__(SF_G) void sos_apply_kernel(const float* in, long ld_in, const int* n, int n_max, const double* sos,
                                                         const double* ws, int C, float* out, long ld_out) {
  __shared__ float lds[SF_G * SF_LDP];
  const int lane = threadIdx.x, b = blockIdx.y, base = blockIdx.x * (SF_G * SF_L);
  const int n_b = sf_row_len(n, b, n_max);
  double c[S][5];
  const bool ident = sf_coeffs<S>(sos, b, c);
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const int len = min(max(n_b - (base + lane * SF_L), 0), SF_L);
  double z[S][2];
#pragma unroll
  for (int s = 0; s < S; ++s) z[s][0] = z[s][1] = 0.0;
  const int ch = blockIdx.x * SF_G + lane;
  if (!ident && ch < C && len > 0) {
    const double* w = ws + ((long)b * C + ch) * (2 * S);
#pragma unroll
    for (int s = 0; s < S; ++s) { z[s][0] = w[2 * s]; z[s][1] = w[2 * s + 1]; }
  }
  float pre[SF_P];
  sf_load_piece(row, base, 0, n_b, lane, pre);
#pragma unroll 1
  for (int p = 0; p < SF_L / SF_P; ++p) {
    sf_piece_to_lds(lds, lane, pre);  // (0 at and behind n_b)
    __syncthreads();
    if (p + 1 < SF_L / SF_P) sf_load_piece(row, base, p + 1, n_b, lane, pre);
    if (!ident) {  // uniform.  An identity row keeps the staged bits: 1 * -0.0 + 0.0 would lose the sign of zero
#pragma unroll 4
      for (int j = 0; j < SF_P; ++j) {
        float y = 0.f;
        if (p * SF_P + j < len) y = (float)sf_step<S>(c, z, (double)lds[lane * SF_LDP + j]);
        lds[lane * SF_LDP + j] = y;
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < SF_P; ++k) {
      const int e = lane + SF_G * k;
      const int i = base + (e / SF_P) * SF_L + p * SF_P + (e % SF_P);
      if (i < n_max) orow[i] = lds[(e / SF_P) * SF_LDP + (e % SF_P)];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
extern "C" int wft_sos_filter_chunk(void) { return SF_L; }
extern "C" int wft_sos_filter_group(void) { return SF_G; }

extern "C" int64_t wft_sos_filter_workspace_bytes(int B, int64_t n_max, int S) {
  if (B < 1 || B > 65535 || n_max < 1 || n_max > SF_MAX_N || S < 1 || S > SF_MAX_S) return -1;
  return (int64_t)B * cdiv64(n_max, SF_L) * (2 * S) * (int64_t)sizeof(double);
}

template <int S>
static int sf_launch(const float* in, int64_t ld_in, const int32_t* n, int n_max, const double* sos, float* out, int64_t ld_out,
                     double* ws, int B, hipStream_t st) {
  const int C = (int)cdiv64(n_max, SF_L), groups = (int)cdiv64(n_max, (int64_t)SF_G * SF_L);
  hipLaunchKernelGGL(sos_local_kernel<S>, dim3(groups, B), dim3(SF_G), 0, st, in, (long)ld_in, n, n_max, sos, ws, C);
  hipLaunchKernelGGL(sos_scan_kernel<S>, dim3(B), dim3(64), 0, st, n, n_max, sos, ws, C);
  hipLaunchKernelGGL(sos_apply_kernel<S>, dim3(groups, B), dim3(SF_G), 0, st, in, (long)ld_in, n, n_max, sos, (const double*)ws, C, out,
                     (long)ld_out);
  WFT_CHECK_LAUNCH_AS("wft_sos_filter_f32");
  return WFT_OK;
}

extern "C" int wft_sos_filter_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* sos, int S, float* out,
                                  int64_t ld_out, void* workspace, int64_t workspace_bytes, int B, void* stream) {
  WFT_CHECK_ARG(in && sos && out && workspace, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= SF_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(S >= 1 && S <= SF_MAX_S, "1 to 4 sections");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG(workspace_bytes >= wft_sos_filter_workspace_bytes(B, n_max, S), "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)sos % 8 == 0 &&
                    (uintptr_t)workspace % 8 == 0,
                "in / out / n must be 4-byte, sos / workspace 8-byte aligned");
  if (!(in == out && ld_in == ld_out)) {  // in place is the same pointer and the same stride; anything else must not overlap
    const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (B - 1) * ld_in + n_max);
    const uintptr_t o0 = (uintptr_t)out, o1 = (uintptr_t)(out + (B - 1) * ld_out + n_max);
    WFT_CHECK_ARG(i1 <= o0 || o1 <= i0, "in and out overlap partially");
  }
  hipStream_t st = (hipStream_t)stream;
  switch (S) {
    case 1: return sf_launch<1>(in, ld_in, n, (int)n_max, sos, out, ld_out, (double*)workspace, B, st);
    case 2: return sf_launch<2>(in, ld_in, n, (int)n_max, sos, out, ld_out, (double*)workspace, B, st);
    case 3: return sf_launch<3>(in, ld_in, n, (int)n_max, sos, out, ld_out, (double*)workspace, B, st);
    default: return sf_launch<4>(in, ld_in, n, (int)n_max, sos, out, ld_out, (double*)workspace, B, st);
  }
}
