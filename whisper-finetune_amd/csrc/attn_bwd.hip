// attn_bwd.hip — the 8-wave backward kernels: every call the one-wave-per-SIMD kernels (attn_dq4w.hip, attn_dkdv4w.hip) do not take
#include "attn_common.h"
// ------------------------------------------------------------------------------ delta
// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d] and lse enter both backward kernels NEGATED, as the initial accumulators of the
// dP and S MFMA chains (S' = S - lse / scale, so exp2(c S') = exp(scale S - lse) needs no subtraction; dP' = dP - delta).
// Round 3: there is no delta kernel any more.  A lane of the dQ kernel already holds half of its query's dO row for the dP
// product; it loads the same half of the O row, forms its 32 products, adds its partner lane's (the other half: lane ^ 32) and
// has -delta; it writes both constants to the workspace for the dK/dV kernel, which runs behind it on the stream (96 launches and
// a second pass over O and dO per step less: 3.6 ms at 68 clips).

// ------------------------------------------------------------------------------ dQ
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[32768];  // [buf 2][K 8K | V 8K]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: conditions on it are scalar branches, not exec masks
  const int r = lane & 31, h = lane >> 5;
  int bx, hd, b;
  att_block_coords((p.Tq + 127) >> 7, p.H, p.B, p.xcd, bx, hd, b);
  const int q0 = bx * 128;
  const int qw0 = q0 + wave * 32;
  const int qi = qw0 + r;
  const int qc = qi < p.Tq ? qi : p.Tq - 1;
  const unsigned short* qrow = p.q + (long)b * p.q_bs + (long)qc * p.ldq + hd * 64;
  const unsigned short* dorow = p.d_o + (long)b * p.do_bs + (long)qc * p.lddo + hd * 64;
  const unsigned short* kb = p.k + (long)b * p.k_bs + hd * 64;
  const unsigned short* vb = p.v + (long)b * p.v_bs + hd * 64;
  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = att_load_reg_frag(qrow, s, h);
    dof[s] = att_load_reg_frag(dorow, s, h);
  }
  const AttOffs offs = att_offsets(lane);
  const AttStage stK = att_stage_init(p.ldk, wave, lane), stV = att_stage_init(p.ldv, wave, lane);
  const long sidx = ((long)b * p.H + hd) * p.Tq + qc;
  // row constants of this lane's query, negated: the initial accumulators of the S and dP chains
  const float nlse = -p.lse[sidx] / p.ls;
  float ndlt;
  {
    const unsigned short* orow = p.o + (long)b * p.o_bs + (long)qc * p.ldo + hd * 64;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 of = att_load_reg_frag(orow, s, h);
      const u32x4 ou = __builtin_bit_cast(u32x4, of), du = __builtin_bit_cast(u32x4, dof[s]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part += bf2f((unsigned short)(ou[e] & 0xffff)) * bf2f((unsigned short)(du[e] & 0xffff));
        part += bf2f((unsigned short)(ou[e] >> 16)) * bf2f((unsigned short)(du[e] >> 16));
      }
    }
    ndlt = -(part + __shfl_xor(part, 32, 64));  // (a + b == b + a: both lanes of a query hold the same bits)
  }
  if (h == 0 && qi < p.Tq) {  // for the dK/dV kernel
    p.delta[sidx] = ndlt;
    p.delta[(long)p.B * p.H * p.Tq + sidx] = nlse;
  }

  int nkt = (p.Tk + 63) >> 6;
  if (p.causal) {
    const int last = (q0 + 127) / 64 + 1;
    nkt = nkt < last ? nkt : last;
  }
  const float c = p.c;
  const f32x16 zero16 = f32x16{0};
  f32x16 dqacc[2];
  dqacc[0] = zero16;
  dqacc[1] = zero16;
  f32x16 sinit, pinit;
#pragma unroll
  for (int e = 0; e < 16; ++e) { sinit[e] = nlse; pinit[e] = ndlt; }

  att_stage2(stK, kb, p.ldk, smem, stV, vb, p.ldv, smem + 8192, 0, p.Tk, wave, lane);
  __syncthreads();

  auto tile = [&](auto cur_tag, int kt) {
    constexpr int CUR = decltype(cur_tag)::value;
    const int key0 = kt * 64;
    if (kt + 1 < nkt) {
      att_stage2(stK, kb, p.ldk, smem + (CUR ^ 1) * 16384, stV, vb, p.ldv, smem + (CUR ^ 1) * 16384 + 8192, key0 + 64, p.Tk,
                 wave, lane);
    }
    const char* kt_l = smem + CUR * 16384;
    const char* vt_l = kt_l + 8192;
    if (qw0 < p.Tq && !(p.causal && key0 > qw0 + 31)) {
      f32x16 sacc[2], pacc[2];
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_row_frag(kt_l, offs, kb2, 0), qf[0], sinit, 0, 0, 0);
        pacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_row_frag(vt_l, offs, kb2, 0), dof[0], pinit, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < 4; ++s) {
          sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_row_frag(kt_l, offs, kb2, s), qf[s], sacc[kb2], 0, 0, 0);
          pacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_row_frag(vt_l, offs, kb2, s), dof[s], pacc[kb2], 0, 0, 0);
        }
      }
      if ((key0 + 64 > p.Tk) || (p.causal && key0 + 63 > qw0)) {
        const int lim = (p.causal ? (qi + 1 < p.Tk ? qi + 1 : p.Tk) : p.Tk) - key0 - 4 * h;
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const bool ok = (32 * kb2 + (e & 3) + 8 * (e >> 2)) < lim;
            const float pv = ok ? __builtin_amdgcn_exp2f(sacc[kb2][e] * c) : 0.f;
            sacc[kb2][e] = pv * pacc[kb2][e];
          }
      } else {
        // packed fp32 (v_pk_mul): two elements per VALU issue slot; the subtractions of lse and delta happened in the MFMAs
        const f32x2 c2 = {c, c};
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            f32x2 t2 = {sacc[kb2][2 * e], sacc[kb2][2 * e + 1]};
            t2 = t2 * c2;
            const f32x2 p2 = {__builtin_amdgcn_exp2f(t2[0]), __builtin_amdgcn_exp2f(t2[1])};
            f32x2 g2 = {pacc[kb2][2 * e], pacc[kb2][2 * e + 1]};
            g2 = g2 * p2;  // dS^T (unscaled)
            sacc[kb2][2 * e] = g2[0];
            sacc[kb2][2 * e + 1] = g2[1];
          }
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 dsf = att_pack8(sacc[ks >> 1], ks & 1);
#pragma unroll
        for (int db = 0; db < 2; ++db)
          dqacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_tr_frag(kt_l, offs, ks, db), dsf, dqacc[db], 0, 0, 0);
      }
    }
    __syncthreads();
  };
  int kt = 0;
  for (; kt + 1 < nkt; kt += 2) {
    tile(IntC<0>{}, kt);
    tile(IntC<1>{}, kt + 1);
  }
  if (kt < nkt) tile(IntC<0>{}, kt);

  if (qi < p.Tq) {
    unsigned short* drow = p.dq + (long)b * p.dq_bs + (long)qi * p.lddq + hd * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int d = 32 * db + 8 * a + 4 * h;
        u32x2 pk = {pack2bf(dqacc[db][4 * a] * p.scale, dqacc[db][4 * a + 1] * p.scale),
                    pack2bf(dqacc[db][4 * a + 2] * p.scale, dqacc[db][4 * a + 3] * p.scale)};
        *(u32x2*)(drow + d) = pk;
      }
  }
  if (p.cs_q && qw0 < p.Tq)  // q-projection bias gradient: this wave's 32 queries, summed per head column
    att_colsum_store(dqacc, p.scale, qi < p.Tq, r, h,
                     p.cs_q + ((long)b * ((p.Tq + 31) >> 5) + (qw0 >> 5)) * (p.H * 64) + hd * 64);
}

// ------------------------------------------------------------------------------ dK, dV
// Per 64-query tile the block stages Q, dO (2 x 8 KiB) AND the tile's 64 lse2 / 64 delta values by LDS-DMA
// (global_load_lds_dword: no VGPR round trip, so no compiler-inserted vmcnt(0) in front of an LDS store — that wait used
// to drain the prefetch of the next tile at the START of every tile).  Transposed Q^T / dO^T reads are inline asm
// issued ahead of the S / dP MFMAs of their 32-query half (hipcc drains all LDS-DMA before a ds_read_tr builtin).
// Query tile of the dK/dV sweep: DKDV_Q queries per stage and barrier.  128 (round 3): half the __syncthreads and half the
// LDS-DMA issue phases per MFMA of the 64-query tiles (in-kernel stamps of round 1: 435 + 325 of 4 819 cycles per 64-query tile).
#define DKDV_Q 128
#define DKDV_BUF (2 * DKDV_Q * 128 + 2 * DKDV_Q * 4)  // Q [DKDV_Q][64] bf16 | dO | -lse/scale f32 [DKDV_Q] | -delta
__device__ __forceinline__ void glds4(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const WFT_GLB void*)gsrc, (WFT_LDS void*)lds_wave_base, 4, 0, 0);
}
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(AttnP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [buf 2][Q | dO | -lse/scale | -delta], 2 * DKDV_BUF bytes
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: conditions on it are scalar branches, not exec masks
  const int r = lane & 31, h = lane >> 5;
  int bx, hd, b;
  att_block_coords((p.Tk + 127) >> 7, p.H, p.B, p.xcd, bx, hd, b);
  const int k0 = bx * 128;
  const int kw0 = k0 + wave * 32;
  const int ki = kw0 + r;
  const int kc = ki < p.Tk ? ki : p.Tk - 1;
  const unsigned short* krow = p.k + (long)b * p.k_bs + (long)kc * p.ldk + hd * 64;
  const unsigned short* vrow = p.v + (long)b * p.v_bs + (long)kc * p.ldv + hd * 64;
  const unsigned short* qb = p.q + (long)b * p.q_bs + hd * 64;
  const unsigned short* dob = p.d_o + (long)b * p.do_bs + hd * 64;
  const long sbase = ((long)b * p.H + hd) * p.Tq;
  const float* dlt_b = p.delta + sbase;
  const float* lse_b = p.delta + (long)p.B * p.H * p.Tq + sbase;  // -lse / scale, written (like -delta) by the dQ kernel, which runs first
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = att_load_reg_frag(krow, s, h);
    vf[s] = att_load_reg_frag(vrow, s, h);
  }
  const AttOffs offs = att_offsets(lane);
  const AttStage stQ = att_stage_init(p.ldq, wave, lane), stDO = att_stage_init(p.lddo, wave, lane);
  const unsigned lds0 = lds_addr_of(smem);
  // one base register set per buffer (the offsets inside a buffer ride in the instructions' 16-bit immediates)
  unsigned tra[2][2][2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int t = 0; t < 2; ++t) tra[cb][db][t] = lds0 + cb * DKDV_BUF + offs.tr[db][t];
  unsigned rowa[2][4];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int s = 0; s < 4; ++s) rowa[cb][s] = lds0 + cb * DKDV_BUF + offs.row[s];
  const unsigned rca = lds0 + 16 * h;  // this lane's first row constant: query 4 h of a 32-query half (+ buffer, + 32 a via immediates)
  const float c = p.c;
  const f32x2 c2 = {c, c};
  const int nqt = (p.Tq + DKDV_Q - 1) / DKDV_Q;
  const int qt0 = p.causal ? (k0 / DKDV_Q) : 0;  // first query tile that can see key k0
  const f32x16 zero16 = f32x16{0};
  f32x16 dkacc[2], dvacc[2];
  dkacc[0] = zero16; dkacc[1] = zero16;
  dvacc[0] = zero16; dvacc[1] = zero16;

  auto stage_q = [&](char* base, int qt) {
#pragma unroll
    for (int cq = 0; cq < DKDV_Q / 64; ++cq)
      if (qt * DKDV_Q + cq * 64 < p.Tq)  // (a 64-row chunk wholly past the sequence end is neither staged nor read)
        att_stage2(stQ, qb, p.ldq, base + cq * 8192, stDO, dob, p.lddo, base + DKDV_Q * 128 + cq * 8192, qt * DKDV_Q + cq * 64, p.Tq, wave, lane);
    // row constants: wave w stages 64 values — even waves -lse/scale, odd waves -delta, of queries 64 (w >> 1) .. (rows clamped;
    // out-of-range rows are masked later)
    if (wave < DKDV_Q / 32) {
      int qq = qt * DKDV_Q + (wave >> 1) * 64 + lane;
      qq = qq < p.Tq ? qq : p.Tq - 1;
      glds4(((wave & 1) == 0 ? lse_b : dlt_b) + qq, base + 2 * DKDV_Q * 128 + (wave & 1) * (DKDV_Q * 4) + (wave >> 1) * 256);
    }
  };

  if (qt0 < nqt) {
    stage_q(smem, qt0);
    __syncthreads();
  }
  auto tile = [&](auto cur_tag, int qt) {
    constexpr int CUR = decltype(cur_tag)::value;
    const int qq0 = qt * DKDV_Q;
    if (qt + 1 < nqt) stage_q(smem + (CUR ^ 1) * DKDV_BUF, qt + 1);
    if (kw0 < p.Tk && !(p.causal && kw0 > qq0 + DKDV_Q - 1)) {  // (a wave whose 32 keys lie past the end only stages)
      static_for<DKDV_Q / 32>([&](auto qb_tag) {
        constexpr int QB2 = decltype(qb_tag)::value;
        constexpr int qb2 = QB2;
        // a 32-query half that lies entirely past the sequence end or above the causal diagonal contributes nothing
        if (qq0 + 32 * qb2 >= p.Tq || (p.causal && kw0 > qq0 + 32 * qb2 + 31)) return;
        // transposed fragments of this 32-query half: in flight under the S / dP MFMAs and the exponentials
        s16x4 dot[2][2][2], qt_[2][2][2];
        static_for<2>([&](auto ks_tag) {
          constexpr int ks = decltype(ks_tag)::value;
#pragma unroll
          for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              dot[ks][db][t] = att_tr_asm<DKDV_Q * 128 + (2 * QB2 + ks) * 2048>(tra[CUR][db][t]);
              qt_[ks][db][t] = att_tr_asm<(2 * QB2 + ks) * 2048>(tra[CUR][db][t]);
            }
        });
        // all eight Q / dO row fragments of the half in one batch behind the transposed reads: ONE LDS round trip in front of
        // the S / dP MFMAs instead of one per k-step (the reads used to be issued pairwise, each pair waited for on the spot)
        bf16x8 aq[4], ad[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          aq[s] = att_row_asm<QB2 * 4096>(rowa[CUR][s]);
          ad[s] = att_row_asm<DKDV_Q * 128 + QB2 * 4096>(rowa[CUR][s]);
        }
        // the half's row constants -lse / scale and -delta: the 16 values a lane needs (queries 8 a + 4 h + e) are laid out
        // exactly like the f32x16 C operand, so they ARE the initial accumulators of the S and dP chains (no VALU at all)
        f32x4 l4[4], d4[4];
        static_for<4>([&](auto a_tag) {
          constexpr int a = decltype(a_tag)::value;
          l4[a] = att_f4_asm<2 * DKDV_Q * 128 + 128 * QB2 + 32 * a>(rca + CUR * DKDV_BUF);
          d4[a] = att_f4_asm<2 * DKDV_Q * 128 + DKDV_Q * 4 + 128 * QB2 + 32 * a>(rca + CUR * DKDV_BUF);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        f32x16 sinit, pinit;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e) { sinit[4 * a + e] = l4[a][e]; pinit[4 * a + e] = d4[a][e]; }
        f32x16 sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[0], kf[0], sinit, 0, 0, 0);
        f32x16 pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[0], vf[0], pinit, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < 4; ++s) {
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[s], kf[s], sacc, 0, 0, 0);
          pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[s], vf[s], pacc, 0, 0, 0);
        }
        f32x16 dsacc;
        // one decision per 32-query half (wave-uniform): the unmasked body is a single basic block — its eight lse / delta
        // reads, 32 exponentials and the packed arithmetic can be scheduled against each other
        const bool need_mask = (qq0 + 32 * qb2 + 32 > p.Tq) || (kw0 + 32 > p.Tk) || (p.causal && kw0 + 31 > qq0 + 32 * qb2);
        if (need_mask) {
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int qg = qq0 + 32 * qb2 + 8 * a + 4 * h + e;
              const bool ok = qg < p.Tq && ki < p.Tk && !(p.causal && ki > qg);
              const float pv = ok ? __builtin_amdgcn_exp2f(sacc[4 * a + e] * c) : 0.f;
              sacc[4 * a + e] = pv;
              dsacc[4 * a + e] = ok ? pv * pacc[4 * a + e] : 0.f;
            }
        } else {
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 4; e += 2) {  // packed fp32 pairs
              f32x2 t2 = {sacc[4 * a + e], sacc[4 * a + e + 1]};
              t2 = t2 * c2;
              const f32x2 p2 = {__builtin_amdgcn_exp2f(t2[0]), __builtin_amdgcn_exp2f(t2[1])};
              f32x2 g2 = {pacc[4 * a + e], pacc[4 * a + e + 1]};
              g2 = g2 * p2;
              sacc[4 * a + e] = p2[0];
              sacc[4 * a + e + 1] = p2[1];
              dsacc[4 * a + e] = g2[0];
              dsacc[4 * a + e + 1] = g2[1];
            }
        }
        bf16x8 pf[2], dsf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          pf[ks] = att_pack8(sacc, ks);
          dsf[ks] = att_pack8(dsacc, ks);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dvacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_join(dot[ks][db][0], dot[ks][db][1]), pf[ks], dvacc[db], 0, 0, 0);
            dkacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_join(qt_[ks][db][0], qt_[ks][db][1]), dsf[ks], dkacc[db], 0, 0, 0);
          }
      });
    }
    __syncthreads();
  };
  int qt = qt0;
  for (; qt + 1 < nqt; qt += 2) {
    tile(IntC<0>{}, qt);
    tile(IntC<1>{}, qt + 1);
  }
  if (qt < nqt) tile(IntC<0>{}, qt);

  if (ki < p.Tk) {
    unsigned short* dkrow = p.dk + (long)b * p.dk_bs + (long)ki * p.lddk + hd * 64;
    unsigned short* dvrow = p.dv + (long)b * p.dv_bs + (long)ki * p.lddv + hd * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int d = 32 * db + 8 * a + 4 * h;
        u32x2 pk = {pack2bf(dkacc[db][4 * a] * p.ls, dkacc[db][4 * a + 1] * p.ls),
                    pack2bf(dkacc[db][4 * a + 2] * p.ls, dkacc[db][4 * a + 3] * p.ls)};
        *(u32x2*)(dkrow + d) = pk;
        u32x2 pv = {pack2bf(dvacc[db][4 * a], dvacc[db][4 * a + 1]),
                    pack2bf(dvacc[db][4 * a + 2], dvacc[db][4 * a + 3])};
        *(u32x2*)(dvrow + d) = pv;
      }
  }
  if (p.cs_v && kw0 < p.Tk)  // v-projection bias gradient
    att_colsum_store(dvacc, 1.0f, ki < p.Tk, r, h, p.cs_v + ((long)b * ((p.Tk + 31) >> 5) + (kw0 >> 5)) * (p.H * 64) + hd * 64);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
void wft_attn_dq8w_launch(const AttnP& p, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), 0, s, p);
}
int wft_attn_dkdv8w_launch(const AttnP& p, dim3 grid, hipStream_t s) {
  // (160 KiB of LDS per CU: gfx950)
  return wft_launch_lds<attn_bwd_dkdv_kernel>(grid, dim3(256), 2 * DKDV_BUF, s, p);
}
