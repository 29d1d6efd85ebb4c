// ECDSA P-256 verification with TWO LANES PER SIGNATURE (device only) - the small-batch variant of p256_verify29.h.
//
// Same algorithm, same gates, same window recodings, same tables as p256_verify_core29 (which it must agree with bit for
// bit: tests/test_gpu_parity.py runs both against the oracle); what changes is the shape of the instruction stream.  A
// 30 000-signature block is 469 wavefronts on 1024 SIMDs and one wave issues one VALU instruction per ~4.2 cycles, so the
// kernel time is the LENGTH of the per-wave stream.  Lanes 2k (E) and 2k+1 (O) share signature k: the point operations are
// the generated programs of pair29_gcn.h (732 / 1364 / 1104 instructions for dbl / add / madd - round 6; one lane: 1201 / 2374 / 1642),
// every field product is executed by both lanes on different operands, limbs cross lanes with DPP quad_perm:[1,0,3,2].
// Between operations  E holds A = X, B = Y  and  O holds B = Z.  The scalar part (gates, s^-1 mod n, u1, u2, digits) is
// computed redundantly by both lanes.
//
// Replaces crypto/ecdsa.Verify reached from bccsp/sw/ecdsa.go:56.
#pragma once
#include "p256_verify29.h"
#include "p256_odd4.h"
#include "pair29_gcn.h"

namespace fab {

struct pair_pt {
    fe A, B;   // E: X, Y      O: don't-care, Z
};

__device__ __forceinline__ int32_t pair_swap_i32(int32_t v) {   // partner lane's value (quad_perm:[1,0,3,2])
    return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ void pair_swap_fe(fe& r, const fe& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = pair_swap_i32(a.v[i]);
}
__device__ __forceinline__ void pair_sel(pair_pt& r, bool c, const pair_pt& a, const pair_pt& b) {
    fe_sel(r.A, c, a.A, b.A);
    fe_sel(r.B, c, a.B, b.B);
}

#define PAIR_TMPS __attribute__((unused)) fe tU1, tU2, tU3, tU4, tU6, tW, tH, tRR, tP1, tP2, tT0, tT1, tTD
#define PAIR_DBL(P) PAIR29_DBL((P).A, (P).B, tU1, tU2, tU3, tW, tP1, tP2, tT0, tT1, tTD)
// Four doublings as one generated program (round 8: the doublings of a 4-bit window); tW is its second B register.
#define PAIR_DBL4(P) PAIR29_DBL4((P).A, (P).B, tU1, tU2, tU3, tP1, tT0, tTD, tW)
#define PAIR_ADD(R, P, C, D) PAIR29_ADD((R).A, (R).B, (P).A, (P).B, tH, tRR, tW, tU1, tU2, tU3, tU4, tU6, tP1, tP2, tT0, tT1, tTD, C, D)
#define PAIR_MADD(R, P, C, D) PAIR29_MADD((R).A, (R).B, (P).A, (P).B, tU1, tU2, tU3, tU4, tH, tRR, tP1, tP2, tT0, tT1, tTD, C, D)
// The co-Z table build (round 10).  PAIR_DBLU: P <- 2P, and for an affine P (Z = 1) the point itself over the double's Z in (QX, QY) on E.
// PAIR_ZADDU: R <- (DX, DY) + P for two points over P's Z, and (NDX, NDY) <- (DX, DY) over R's Z.
#define PAIR_DBLU(P, QX, QY) PAIR29_DBLU((P).A, (P).B, QX, QY, tU1, tU3, tW, tP1, tP2, tT0, tT1, tTD)
#define PAIR_ZADDU(R, NDX, NDY, P, DX, DY) PAIR29_ZADDU((R).A, (R).B, NDX, NDY, (P).A, (P).B, DX, DY, tH, tRR, tU1, tP1, tP2, tT0, tT1, tW, tTD)

// Per-signature table j*Q (j = 1..16) in the global workspace.  Per workgroup slot: [entry][q 0..7][pair NP] x 16 bytes;
// q 0..4 = X[9] Y[9] pad, q 5..7 = Z[9] pad.  E stores / owns the X,Y quads, O the Z quads.
// Layout (FABGPU_QTAB_SIG_MAJOR, the default): per SIGNATURE contiguous - entry j of signature k is the 128-byte line
// slot + (k * 16 + j - 1) * 128: the gather of a window (both lanes of the pair, eight 16-byte cells) is exactly one cache line, fully
// used.  The round-1 layout [entry][q][pair] made the STORES of a wave contiguous but scattered a wave's gather over ~27 lines of which
// 16 bytes each were wanted: rocprofv3 FETCH_SIZE 418 MB per 30 000-tuple launch for 266 MB of useful bytes (profiles/r01_pmc_traffic.json).
#ifndef FABGPU_QTAB_SIG_MAJOR
#define FABGPU_QTAB_SIG_MAJOR 1
#endif
template <int NP>
struct PairQTab {
    uint4* pair;   // first 16-byte cell of this signature's table
    // slot: workspace of this workgroup slot (NP signatures x 16 entries x 8 cells); k: index of the signature inside the workgroup
    static __device__ __forceinline__ PairQTab of(uint4* slot, uint32_t k) {
#if FABGPU_QTAB_SIG_MAJOR
        return PairQTab{slot + (size_t)k * (16 * 8)};
#else
        return PairQTab{slot + k};
#endif
    }
#if FABGPU_QTAB_SIG_MAJOR
    __device__ __forceinline__ uint4* cell(int j, int q) const { return pair + ((size_t)(j - 1) * 8 + q); }
#else
    __device__ __forceinline__ uint4* cell(int j, int q) const { return pair + ((size_t)(j - 1) * 8 + q) * NP; }
#endif
    __device__ __forceinline__ void store_state(int j, const pair_pt& p, bool odd) const {
        if (!odd) {
            *cell(j, 0) = make_uint4(p.A.v[0], p.A.v[1], p.A.v[2], p.A.v[3]);
            *cell(j, 1) = make_uint4(p.A.v[4], p.A.v[5], p.A.v[6], p.A.v[7]);
            *cell(j, 2) = make_uint4(p.A.v[8], p.B.v[0], p.B.v[1], p.B.v[2]);
            *cell(j, 3) = make_uint4(p.B.v[3], p.B.v[4], p.B.v[5], p.B.v[6]);
            *cell(j, 4) = make_uint4(p.B.v[7], p.B.v[8], 0, 0);
        } else {
            *cell(j, 5) = make_uint4(p.B.v[0], p.B.v[1], p.B.v[2], p.B.v[3]);
            *cell(j, 6) = make_uint4(p.B.v[4], p.B.v[5], p.B.v[6], p.B.v[7]);
            *cell(j, 7) = make_uint4(p.B.v[8], 0, 0, 0);
        }
    }
    // five 16-byte loads, the same code on both lanes: E reads q = q0 + k clamped to 7, O reads q = k
    __device__ __forceinline__ void load5(uint32_t j, int q0, uint4 (&l)[5]) const {
#pragma unroll
        for (int k = 0; k < 5; k++) {
            int q = q0 + k;
            l[k] = *cell((int)j, q > 7 ? 7 : q);
        }
    }
    // state layout: E gets (X, Y), O gets B = Z
    __device__ __forceinline__ void load_state(uint32_t j, pair_pt& p, bool odd) const {
        uint4 l[5];
        load5(j, odd ? 5 : 0, l);
        p.A.v[0] = l[0].x; p.A.v[1] = l[0].y; p.A.v[2] = l[0].z; p.A.v[3] = l[0].w;
        p.A.v[4] = l[1].x; p.A.v[5] = l[1].y; p.A.v[6] = l[1].z; p.A.v[7] = l[1].w;
        p.A.v[8] = l[2].x;
        fe y;
        y.v[0] = l[2].y; y.v[1] = l[2].z; y.v[2] = l[2].w;
        y.v[3] = l[3].x; y.v[4] = l[3].y; y.v[5] = l[3].z; y.v[6] = l[3].w;
        y.v[7] = l[4].x; y.v[8] = l[4].y;
        fe_sel(p.B, odd, p.A, y);       // O: the first nine words it read are Z
    }
    // crossed layout for PAIR_ADD: E gets C = Z2, O gets C = X2, D = Y2 (E's D is garbage)
    __device__ __forceinline__ void load_crossed(uint32_t j, fe& C, fe& D, bool odd) const {
        uint4 l[5];
        load5(j, odd ? 0 : 5, l);
        C.v[0] = l[0].x; C.v[1] = l[0].y; C.v[2] = l[0].z; C.v[3] = l[0].w;
        C.v[4] = l[1].x; C.v[5] = l[1].y; C.v[6] = l[1].z; C.v[7] = l[1].w;
        C.v[8] = l[2].x;
        D.v[0] = l[2].y; D.v[1] = l[2].z; D.v[2] = l[2].w;
        D.v[3] = l[3].x; D.v[4] = l[3].y; D.v[5] = l[3].z; D.v[6] = l[3].w;
        D.v[7] = l[4].x; D.v[8] = l[4].y;
    }
};

// The same table in LDS, EIGHT entries per signature (the odd multiples (2j - 1) Q, j = 1..8, for the all-odd 4-bit recoding of
// pair_u2_mult_odd29 - or j*Q for the Booth form, 65 windows, of FABGPU_FLAG_PAIR_BOOTH4): 128 signatures x 8 x 128 B = 128 KiB of
// the CU's 160 KiB - the pair kernel runs one workgroup per CU anyway.  Costs 11 more additions per verification than the 16-entry
// table with 5-bit windows (63 instead of 52) and saves eight table-building operations; in exchange NOTHING of the
// per-signature table touches the memory system: the global-workspace form writes 60 MB and fetches 2 x 110 MB per 30 000-tuple
// launch (58x the algorithmic bytes), which is free on an idle chip and costs 4-17 % beside a tenant that streams 1.5-5 TB/s
// (tools/gpu_hbm_tenant_probe.py).  A signature's entries are 65 cells apart (one cell of padding per signature): a wave's 32 pairs
// gather from 32 different signatures, and a 1 KiB stride would put them all on the same banks.
constexpr int PAIR_LDS_ENTRIES = 8;
constexpr int PAIR_LDS_CELLS_PER_SIG = PAIR_LDS_ENTRIES * 8 + 1;
struct PairQTabLds {
    uint4* pair;   // (LDS) first cell of this signature's table
    static __device__ __forceinline__ PairQTabLds of(uint4* lds, uint32_t k) { return PairQTabLds{lds + (size_t)k * PAIR_LDS_CELLS_PER_SIG}; }
    __device__ __forceinline__ uint4* cell(int j, int q) const { return pair + ((j - 1) * 8 + q); }
    __device__ __forceinline__ void store_state(int j, const pair_pt& p, bool odd) const {
        if (!odd) {
            *cell(j, 0) = make_uint4(p.A.v[0], p.A.v[1], p.A.v[2], p.A.v[3]);
            *cell(j, 1) = make_uint4(p.A.v[4], p.A.v[5], p.A.v[6], p.A.v[7]);
            *cell(j, 2) = make_uint4(p.A.v[8], p.B.v[0], p.B.v[1], p.B.v[2]);
            *cell(j, 3) = make_uint4(p.B.v[3], p.B.v[4], p.B.v[5], p.B.v[6]);
            *cell(j, 4) = make_uint4(p.B.v[7], p.B.v[8], 0, 0);
        } else {
            *cell(j, 5) = make_uint4(p.B.v[0], p.B.v[1], p.B.v[2], p.B.v[3]);
            *cell(j, 6) = make_uint4(p.B.v[4], p.B.v[5], p.B.v[6], p.B.v[7]);
            *cell(j, 7) = make_uint4(p.B.v[8], 0, 0, 0);
        }
        // the partner lane reads what this lane wrote (and the other way round): same wavefront, in-order LDS - only the compiler
        // must not move accesses across
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ void load5(uint32_t j, int q0, uint4 (&l)[5]) const {
#pragma unroll
        for (int k = 0; k < 5; k++) {
            int q = q0 + k;
            l[k] = *cell((int)j, q > 7 ? 7 : q);
        }
    }
    __device__ __forceinline__ void load_state(uint32_t j, pair_pt& p, bool odd) const {
        uint4 l[5];
        load5(j, odd ? 5 : 0, l);
        p.A.v[0] = l[0].x; p.A.v[1] = l[0].y; p.A.v[2] = l[0].z; p.A.v[3] = l[0].w;
        p.A.v[4] = l[1].x; p.A.v[5] = l[1].y; p.A.v[6] = l[1].z; p.A.v[7] = l[1].w;
        p.A.v[8] = l[2].x;
        fe y;
        y.v[0] = l[2].y; y.v[1] = l[2].z; y.v[2] = l[2].w;
        y.v[3] = l[3].x; y.v[4] = l[3].y; y.v[5] = l[3].z; y.v[6] = l[3].w;
        y.v[7] = l[4].x; y.v[8] = l[4].y;
        fe_sel(p.B, odd, p.A, y);
    }
    __device__ __forceinline__ void load_crossed(uint32_t j, fe& C, fe& D, bool odd) const {
        uint4 l[5];
        load5(j, odd ? 0 : 5, l);
        C.v[0] = l[0].x; C.v[1] = l[0].y; C.v[2] = l[0].z; C.v[3] = l[0].w;
        C.v[4] = l[1].x; C.v[5] = l[1].y; C.v[6] = l[1].z; C.v[7] = l[1].w;
        C.v[8] = l[2].x;
        D.v[0] = l[2].y; D.v[1] = l[2].z; D.v[2] = l[2].w;
        D.v[3] = l[3].x; D.v[4] = l[3].y; D.v[5] = l[3].z; D.v[6] = l[3].w;
        D.v[7] = l[4].x; D.v[8] = l[4].y;
    }
};

// E gets x2, O gets y2 of comb entry (window, digit) in the SAME nine registers (they are passed as both C and D of PAIR_MADD)
template <class Tab>
__device__ __forceinline__ void pair_comb_load(const int32_t* __restrict__ tab, int window, uint32_t digit, bool odd, fe& xy) {
    const int32_t* e = tab + Tab::index(window, digit) + (odd ? 9 : 0);
#pragma unroll
    for (int l = 0; l < 9; l++) xy.v[l] = e[l];
}

// w = x^-1 mod M on a lane pair (modinv30.h).  The 30 division steps of a batch are computed by both lanes (round 6: each with one
// column of the transition matrix); then the EVEN
// lane applies the transition matrix to (f, g) and the ODD lane to (d, e) - one update per lane per batch instead of two.
// Both run the (d, e) update code: for (f, g) the modulus correction is forced to zero (t (f, g) is divisible by 2^30 by
// construction, so the same shift is exact).  The result is returned on both lanes.
__device__ __forceinline__ void pair_modinv(u256& out, const u256& x, const modinv_info& mi, bool odd) {
    s30 a, b;                      // E: (f, g)      O: (d, e)
    s30 gx;
    s30_from_u256(gx, x);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.v[i] = odd ? 0 : mi.modulus.v[i];
        b.v[i] = odd ? (i == 0 ? 1 : 0) : gx.v[i];
    }
    int32_t zeta = -1;
#pragma unroll 1
    for (int it = 0; it < 20; it++) {
        if (it >= 17) {      // (modinv30.h modinv: random inputs are done after 17 or 18 batches; g lives on the even lanes)
            uint32_t nz = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) nz |= (uint32_t)b.v[i];
            if (!__any(!odd && nz != 0)) break;
        }
        int32_t fo = pair_swap_i32(a.v[0]), go = pair_swap_i32(b.v[0]);
        uint32_t f0 = (uint32_t)(odd ? fo : a.v[0]), g0 = (uint32_t)(odd ? go : b.v[0]);
        // the division steps with one column of the transition matrix per lane - E: (u, q) from (1, 0), O: (v, r) from (0, 1) - then exchanged
        int32_t ca0 = odd ? 0 : 1, cb0 = odd ? 1 : 0;
        zeta = modinv_divsteps30_column(zeta, f0, g0, ca0, cb0);
        const int32_t pa = pair_swap_i32(ca0), pb = pair_swap_i32(cb0);
        trans2x2 t;
        t.u = odd ? pa : ca0;
        t.q = odd ? pb : cb0;
        t.v = odd ? ca0 : pa;
        t.r = odd ? cb0 : pb;
        // modinv_update_de with the correction masked off on the even lane
        int32_t sa = a.v[8] >> 31, sb = b.v[8] >> 31;
        int32_t ma = (t.u & sa) + (t.v & sb);
        int32_t mb = (t.q & sa) + (t.r & sb);
        int64_t ca = (int64_t)t.u * a.v[0] + (int64_t)t.v * b.v[0];
        int64_t cb = (int64_t)t.q * a.v[0] + (int64_t)t.r * b.v[0];
        ma -= (int32_t)((mi.inv30 * (uint32_t)ca + (uint32_t)ma) & (uint32_t)MI_M30);
        mb -= (int32_t)((mi.inv30 * (uint32_t)cb + (uint32_t)mb) & (uint32_t)MI_M30);
        ma = odd ? ma : 0;
        mb = odd ? mb : 0;
        ca += (int64_t)mi.modulus.v[0] * ma;
        cb += (int64_t)mi.modulus.v[0] * mb;
        ca >>= 30;
        cb >>= 30;
#pragma unroll
        for (int i = 1; i < 9; i++) {
            ca += (int64_t)t.u * a.v[i] + (int64_t)t.v * b.v[i] + (int64_t)mi.modulus.v[i] * ma;
            cb += (int64_t)t.q * a.v[i] + (int64_t)t.r * b.v[i] + (int64_t)mi.modulus.v[i] * mb;
            a.v[i - 1] = (int32_t)((uint32_t)ca & (uint32_t)MI_M30);
            b.v[i - 1] = (int32_t)((uint32_t)cb & (uint32_t)MI_M30);
            ca >>= 30;
            cb >>= 30;
        }
        a.v[8] = (int32_t)ca;
        b.v[8] = (int32_t)cb;
    }
    // E: f = +-1 in a;  O: d in a.  The inverse is d * sign(f): normalise on O, then hand the result to E.
    int32_t fsign_e = a.v[8] >> 31;
    int32_t fsign = pair_swap_i32(fsign_e);       // O: sign of f
    modinv_normalize(a, odd ? fsign : 0, mi);
    u256 w;
    s30_to_u256(w, a);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int32_t o = pair_swap_i32((int32_t)w.w[i]);
        out.w[i] = odd ? w.w[i] : (uint32_t)o;
    }
}

// ecdsa_scalars29 with the inversion shared by the pair, in two parts: w = s^-1 and u2 = r w, then u1 = e w.  The helper wave runs the
// second part after barrier A (round 10: the barrier waits for u2 alone, and u1 is used by the comb behind it and nowhere else).
__device__ __forceinline__ void pair_ecdsa_u2_29(u256& w, u256& u2, const u256& r, const u256& s, bool odd) {
    u256 t;
    {
        const modinv_info NI = MODINV_N_INFO;
        pair_modinv(w, s, NI, odd);
    }
    fn_to_mont(t, r);
    fn_mul(u2, t, w);
}
__device__ __forceinline__ void pair_ecdsa_u1_29(u256& u1, const u256& e, const u256& w) {
    const u256 N = FAB_P256_N;
    u256 ered, t;
    uint32_t br = sub256(t, e, N);
    sel256(ered, br == 0, t, e);
    fn_to_mont(t, ered);
    fn_mul(u1, t, w);
}
__device__ __forceinline__ void pair_ecdsa_scalars29(u256& u1, u256& u2, const u256& e, const u256& r, const u256& s, bool odd) {
    u256 w;
    pair_ecdsa_u2_29(w, u2, r, s, odd);
    pair_ecdsa_u1_29(u1, e, w);
}

// S = k * B over a comb table of B on a lane pair (comb_mult29).  seed: any valid point in pair state.
template <class Tab>
__device__ __forceinline__ void pair_comb_mult29(pair_pt& S, bool& s_inf, const u256& k, const int32_t* __restrict__ tab, const pair_pt& seed,
                                                 bool odd) {
    const fe ONE = {FE29_R1};
    PAIR_TMPS;
    S = seed;
    s_inf = true;
    uint32_t nd = Tab::digit(k, 0);
    fe nxy;
    pair_comb_load<Tab>(tab, 0, nd ? nd : 1u, odd, nxy);
#pragma unroll 1
    for (int i = 0; i < Tab::WINDOWS; i++) {
        uint32_t d = nd;
        fe xy = nxy;
        int inext = i + 1 < Tab::WINDOWS ? i + 1 : i;
        nd = Tab::digit(k, inext);
        pair_comb_load<Tab>(tab, inext, nd ? nd : 1u, odd, nxy);
        pair_pt sum;
        PAIR_MADD(sum, S, xy, xy);
        bool take_ent = s_inf & (d != 0);
        bool take_sum = (!s_inf) & (d != 0);
        pair_sel(S, take_sum, sum, S);
        if (__any(take_ent)) {
            pair_pt ent;
            fe sy;
            pair_swap_fe(sy, xy);           // E: y2
            ent.A = xy;                     // E: x2
            fe_sel(ent.B, odd, ONE, sy);
            pair_sel(S, take_ent, ent, S);
        }
        s_inf = s_inf & (d == 0);
    }
}

// R = S + T on a lane pair with the exceptional cases of the group law (final_add29).
__device__ __forceinline__ void pair_final_add29(pair_pt& Rr, bool& r_inf, const pair_pt& S, bool s_inf, const pair_pt& T, bool t_inf, bool odd) {
    PAIR_TMPS;
    fe C, D, sa, sb;
    pair_swap_fe(sa, T.A);                  // O: X_T
    pair_swap_fe(sb, T.B);                  // E: Z_T    O: Y_T
    fe_sel(C, odd, sa, sb);
    D = sb;
    pair_pt Rp;
    PAIR_ADD(Rp, S, C, D);
    bool hz = fe_is_zero(tH);               // E: h, O: -h
    bool rz_own = fe_is_zero(tRR);          // rr lives on E
    int32_t rz_other = pair_swap_i32(rz_own ? 1 : 0);
    bool rz = odd ? (rz_other != 0) : rz_own;
    r_inf = t_inf & s_inf;
    bool use_T = s_inf & !t_inf;
    bool use_S = t_inf & !s_inf;
    bool both = !s_inf & !t_inf;
    bool use_dbl = both & hz & rz;
    r_inf = r_inf | (both & hz & !rz);
    Rr = Rp;
    if (__any(use_dbl)) {                   // S == T: only a crafted signature gets here - no wavefront of honest ones pays for the doubling
        pair_pt Rd = T;
        PAIR_DBL(Rd);
        pair_sel(Rr, use_dbl, Rd, Rr);
    }
    pair_sel(Rr, use_T, T, Rr);
    pair_sel(Rr, use_S, S, Rr);
}

// R = u1*G + u2*Q on a lane pair.  Q: affine Montgomery (both lanes hold both coordinates).  Returns the pair state of R;
// r_inf as in p256_combined_mult29.  W = width of the signed (Booth) windows over u2: 5 (a 16-entry table j*Q, 52 windows: the
// global-workspace table) or 4 (8 entries, 65 windows: the LDS table).
//
// No addition inside the loop may meet P == +-Q (the addition formulas do not handle it).  Before window i is added T = M Q with M a
// non-zero multiple of 2^W and the addend is d Q, |d| <= 2^(W-1).  M == +-d (mod n) needs M = n +- |d| (M >= 2^W > |d|), possible
// only at the last window, where M = u2 - d: M = n - d gives u2 = n, impossible; M = n + d with d < 0 gives u2 = n - 2|d| and needs
// |d| == n (mod 2^W).  n mod 32 = 17 > 16: never for W = 5.  n mod 16 = 1: for W = 4 EXACTLY ONE scalar, u2 = n - 2
// (digit -1 on top of M = n - 1: T = -Q, addend -Q).  That scalar is recognised up front and its product, -2Q, is taken from the
// table (entry 2, negated) instead of from the loop.
// Per-signature table j*Q, j = 1..2^(W-1), from Q in pair state (first part of pair_combined_mult29).
template <class QTab, int W = 5>
__device__ __forceinline__ void pair_qtab_build29(const pair_pt& Qp, const fe& QX, const fe& QY, const QTab& qtab, bool odd) {
    constexpr int TAB = 1 << (W - 1);
    PAIR_TMPS;
    qtab.store_state(1, Qp, odd);
#pragma unroll 1
    for (int j = 2; j <= TAB; j += 2) {
        pair_pt d;
        qtab.load_state((uint32_t)(j >> 1), d, odd);
        PAIR_DBL(d);
        qtab.store_state(j, d, odd);
        if (j < TAB) {
            pair_pt d1;
            PAIR_MADD(d1, d, QX, QY);
            qtab.store_state(j + 1, d1, odd);
        }
    }
}

// T = u2 * Q over the table pair_qtab_build29 wrote (second part of pair_combined_mult29): NWIN signed W-bit windows, the same
// recoding as p256_combined_mult29 for W = 5, and for W = 4 the scalar u2 = n - 2 (see pair_combined_mult29).
// The four doublings of a 4-bit window are ONE program (PAIR_DBL4) unless DBL1 asks for the per-doubling loop (FABGPU_FLAG_PAIR_DBL1: A/B
// runs and parity tests); the two leave the same point, not the same limbs.
template <class QTab, int W = 5, bool DBL1 = false>
__device__ __forceinline__ void pair_u2_mult29(pair_pt& T, bool& t_inf, const u256& u2, const pair_pt& Qp, const QTab& qtab, bool odd) {
    constexpr int TAB = 1 << (W - 1);                 // entries j*Q, j = 1..TAB
    constexpr int NWIN = (257 + W - 1) / W;           // windows over bits -1 .. 256 of a scalar below n
    PAIR_TMPS;
    uint32_t kw[9];
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = u2.w[i];
    kw[8] = 0;
    T = Qp;
    t_inf = true;
#pragma unroll 1
    for (int i = NWIN - 1; i >= 0; i--) {
        uint32_t field;                               // bits W i - 1 .. W i + W - 1 of the scalar (bit -1 = 0)
        if (i == 0) {
            field = (kw[0] << 1) & ((2u << W) - 1u);
        } else {
            int p = W * i - 1;
            uint64_t two = ((uint64_t)kw[(p >> 5) + 1] << 32) | kw[p >> 5];
            field = (uint32_t)(two >> (p & 31)) & ((2u << W) - 1u);
        }
        int32_t digit = (int32_t)((field >> 1) & (uint32_t)(TAB - 1)) + (int32_t)(field & 1u) - (int32_t)((field >> W) << (W - 1));
        bool neg = digit < 0;
        uint32_t mag = (uint32_t)(neg ? -digit : digit);
        fe C, D;
        qtab.load_crossed(mag ? mag : 1u, C, D, odd);   // issued ahead of the doublings
        if (i != NWIN - 1) {
            if constexpr (W == 4 && !DBL1) {
                PAIR_DBL4(T);
            } else {
#pragma unroll 1
                for (int k = 0; k < W; k++) PAIR_DBL(T);
            }
        }
        {
            const int32_t nm = neg ? -1 : 0, nc = neg ? 1 : 0;        // -y = (y ^ -1) + 1: one v_xad_u32 per limb instead of a negation and a select
#pragma unroll
            for (int l = 0; l < 9; l++) D.v[l] = (D.v[l] ^ nm) + nc;  // -Y2 (lives on O)
        }
        pair_pt sum;
        PAIR_ADD(sum, T, C, D);
        bool take_ent = t_inf & (mag != 0);
        bool take_sum = (!t_inf) & (mag != 0);
        pair_sel(T, take_sum, sum, T);
        if (__any(take_ent)) {   // wave-uniform: only the first non-zero window(s) of a wave convert the entry to state layout
            pair_pt ent;
            fe sc, sd;
            pair_swap_fe(sc, C);            // E: X2     O: Z2
            pair_swap_fe(sd, D);            // E: Y2
            ent.A = sc;
            fe_sel(ent.B, odd, sc, sd);
            pair_sel(T, take_ent, ent, T);
        }
        t_inf = t_inf & (mag == 0);
    }
    if (W == 4) {
        // u2 = n - 2: the one scalar whose last addition is a doubling (see pair_combined_mult29).  (n - 2) Q = -2Q: entry 2, Y negated.
        const u256 NM2 = {{0xFC63254Fu, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu}};
        bool special = true;
#pragma unroll
        for (int l = 0; l < 8; l++) special = special & (u2.w[l] == NM2.w[l]);
        if (__any(special)) {
            pair_pt two;
            qtab.load_state(2u, two, odd);
            fe ny;
#pragma unroll
            for (int l = 0; l < 9; l++) ny.v[l] = -two.B.v[l];
            fe_sel(two.B, odd, two.B, ny);        // E holds Y in B (negate it), O holds Z in B (keep it)
            pair_sel(T, special, two, T);
        }
    }
}

// The LDS table for the all-odd recoding (p256_odd4.h): slot j = (2j - 1) Q, j = 1..8 - eight entries like pair_qtab_build29<4>'s.
// By co-Z additions (round 10; gen_pair_gcn.py has the formulas): slot 1 = Q; one doubling with update leaves D = 2Q and Q over the
// same Z = 2y; then seven times  slot j = slot j-1 + D  with both over one Z, which also re-expresses D over the sum's Z for the next
// step: four product steps where the general addition takes eight.  D lives in registers (X and Y on the even lane; its Z is the
// current entry's) - no slot is borrowed.  The entries are states like any other: every consumer reads them as before.
// Exceptional inputs.  The co-Z addition degenerates only for X1 = X2 over the common Z, i.e. (2j - 3) Q = +-2Q, (2j - 1) Q or
// (2j - 5) Q the point at infinity with 2j - 1 <= 15: impossible for a Q on the curve, whose order is the prime n > 15.  A Q off the
// curve (or out of the field) is refused by the curve gate and its row's status comes from the gate, not from the table.  The programs
// are branch-free and compute no address from data: such a row leaves garbage entries in its own slots and nothing else.
// TABLE_ADD (FABGPU_FLAG_PAIR_TABLE_ADD: A/B runs and parity tests) keeps the build by general additions it replaces, below.
template <class QTab>
__device__ __forceinline__ void pair_qtab_build_odd29(const pair_pt& Qp, const QTab& qtab, bool odd) {
    PAIR_TMPS;
    qtab.store_state(1, Qp, odd);
    pair_pt d = Qp, cur;                      // d: 2Q, then only a carrier of (DX, DY)
    fe DX, DY, qy;
    PAIR_DBLU(d, cur.A, qy);                  // E: cur.A, qy = Q over Z(2Q)
    fe_sel(cur.B, odd, d.B, qy);              // cur = Q as a state over Z(2Q)
    DX = d.A;
    DY = d.B;
#pragma unroll 1
    for (int j = 2; j <= PAIR_LDS_ENTRIES; j++) {
        pair_pt sum;
        fe ndx, ndy;
        PAIR_ZADDU(sum, ndx, ndy, cur, DX, DY);
        cur = sum;
        DX = ndx;
        DY = ndy;
        qtab.store_state(j, cur, odd);
    }
}

// The same table by general additions (round 9: the form behind FABGPU_FLAG_PAIR_TABLE_ADD, and the table of the DBL1 instances).
// Slot 1 = Q, D = 2Q, slot 2 = D + Q (mixed), slot j = slot j-1 + D.  2Q waits in slot 8, where every addition reads it in crossed
// layout, until the last addition overwrites it with 15 Q (its load is issued before that store).  None of the additions meets
// P == +-Q: (2j - 3) Q and 2 Q with 2j - 3 <= 13, Q of prime order (anything else fails the curve gate and its row reports that).
template <class QTab>
__device__ __forceinline__ void pair_qtab_build_odd_add29(const pair_pt& Qp, const fe& QX, const fe& QY, const QTab& qtab, bool odd) {
    PAIR_TMPS;
    qtab.store_state(1, Qp, odd);
    pair_pt d = Qp, cur;
    PAIR_DBL(d);
    qtab.store_state(PAIR_LDS_ENTRIES, d, odd);
    PAIR_MADD(cur, d, QX, QY);
    qtab.store_state(2, cur, odd);
#pragma unroll 1
    for (int j = 3; j <= PAIR_LDS_ENTRIES; j++) {
        fe C, D;
        qtab.load_crossed((uint32_t)PAIR_LDS_ENTRIES, C, D, odd);
        pair_pt sum;
        PAIR_ADD(sum, cur, C, D);
        cur = sum;
        qtab.store_state(j, cur, odd);
    }
}

// T = u2 * Q over that table, k = u2_fold_odd(u2): T = entry[h_63], then 63 x (four doublings; one addition).  No digit is zero and T
// is never infinity: no select, no entry conversion inside the loop, nothing to track.
//
// Exceptional additions (the formulas do not handle P == +-Q).  Before window i is added T = M Q, M = 16 P with P the sum of the digits
// above i: P >= 16^m - 15 (16^m - 1)/15 = 1, so M is a POSITIVE multiple of 16; the addend is d Q, d odd, |d| <= 15 < M.  M + d is the
// prefix of k down to window i and the digits below it sum to less than 16^i in magnitude: for i >= 1 the prefix is below 2^252 + 1 and
// M < n - 15: neither M = |d| nor M = n - |d| is possible.  For i = 0, M = k - d with k <= n.  M == d (mod n): k = 2d + t n, k odd
// and 0 < k < 2n give t = 1, so d < 0 and k = n - 2|d|; M = n - |d| is a multiple of 16 and n mod 16 = 1: |d| = 1, k = n - 2.
// M == -d: k = t n, k = n, which only u2 = 0 folds to - and the range gate refuses r = 0.  EXACTLY ONE k, n - 2, reached from u2 = n - 2
// and from u2 = 2 (tests/test_pair_odd_windows_host.py walks the prefixes).  Its product, -2Q (+2Q for u2 = 2), is computed apart
// behind __any: one doubling of entry 0.
template <class QTab, bool DBL1 = false>
__device__ __forceinline__ void pair_u2_mult_odd29(pair_pt& T, const u256& k, const QTab& qtab, bool odd) {
    PAIR_TMPS;
    odd_walk4 wk;
    odd_walk4_start(wk, k);
    {
        const odd_digit top = odd_walk4_next(wk);
        qtab.load_state(top.entry + 1u, T, odd);
        fe ny;
#pragma unroll
        for (int l = 0; l < 9; l++) ny.v[l] = -T.B.v[l];
        fe_sel(T.B, top.neg & !odd, ny, T.B);      // E holds Y in B, O holds Z
    }
#pragma unroll 1
    for (int i = ODD4_WINDOWS - 2; i >= 0; i--) {
        const odd_digit dg = odd_walk4_next(wk);
        fe C, D;
        qtab.load_crossed(dg.entry + 1u, C, D, odd);    // issued ahead of the doublings
        if constexpr (!DBL1) {
            PAIR_DBL4(T);
        } else {
#pragma unroll 1
            for (int j = 0; j < 4; j++) PAIR_DBL(T);
        }
        {
            const int32_t nm = dg.neg ? -1 : 0, nc = dg.neg ? 1 : 0;  // -y = (y ^ -1) + 1, as in pair_u2_mult29
#pragma unroll
            for (int l = 0; l < 9; l++) D.v[l] = (D.v[l] ^ nm) + nc;  // -Y2 (lives on O)
        }
        pair_pt sum;
        PAIR_ADD(sum, T, C, D);
        T = sum;
    }
    {
        const u256 NM2 = {{0xFC63254Fu, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu}};
        bool special = (k.w[0] | 1u) == NM2.w[0];
#pragma unroll
        for (int l = 1; l < 8; l++) special = special & (k.w[l] == NM2.w[l]);
        if (__any(special)) {
            pair_pt two;
            qtab.load_state(1u, two, odd);
            PAIR_DBL(two);
            fe ny;
#pragma unroll
            for (int l = 0; l < 9; l++) ny.v[l] = -two.B.v[l];
            fe_sel(two.B, ((k.w[0] & 1u) == 0) & !odd, ny, two.B);    // k Q = -2Q; the fold's sign turns it back for u2 = 2
            pair_sel(T, special, two, T);
        }
    }
}

// R = u1*G + u2*Q on a lane pair.  Q: affine Montgomery (both lanes hold both coordinates).  Returns the pair state of R;
// r_inf as in p256_combined_mult29.  W = width of the signed (Booth) windows over u2: 5 (a 16-entry table j*Q, 52 windows: the
// global-workspace table) or 4 (8 entries, 65 windows: the LDS table).
//
// No addition inside the loop may meet P == +-Q (the addition formulas do not handle it).  Before window i is added T = M Q with M a
// non-zero multiple of 2^W and the addend is d Q, |d| <= 2^(W-1).  M == +-d (mod n) needs M = n +- |d| (M >= 2^W > |d|), possible
// only at the last window, where M = u2 - d: M = n - d gives u2 = n, impossible; M = n + d with d < 0 gives u2 = n - 2|d| and needs
// |d| == n (mod 2^W).  n mod 32 = 17 > 16: never for W = 5.  n mod 16 = 1: for W = 4 EXACTLY ONE scalar, u2 = n - 2
// (digit -1 on top of M = n - 1: T = -Q, addend -Q).  That scalar is recognised up front and its product, -2Q, is taken from the
// table (entry 2, negated) instead of from the loop.
// W = 4 runs the all-odd recoding over the table of odd multiples (pair_u2_mult_odd29: 63 windows, no zero digit) unless BOOTH4 asks
// for the Booth form above (FABGPU_FLAG_PAIR_BOOTH4: A/B runs and parity tests).
// TABLE_ADD: the table of odd multiples by general additions (pair_qtab_build_odd_add29) instead of co-Z additions; DBL1 implies it.
template <class QTab, int W = 5, bool DBL1 = false, bool BOOTH4 = false, bool TABLE_ADD = false>
__device__ __forceinline__ void pair_combined_mult29(pair_pt& Rr, bool& r_inf, const u256& u1, const u256& u2, const fe& QX, const fe& QY,
                                                     const int32_t* __restrict__ gtab, const QTab& qtab, bool odd) {
    static_assert(W == 4 || W == 5, "signed 4- or 5-bit windows");
    const fe ONE = {FE29_R1};
    pair_pt Qp;
    Qp.A = QX;
    fe_sel(Qp.B, odd, ONE, QY);
    pair_pt T;
    bool t_inf;
    if constexpr (W == 4 && !BOOTH4) {
        if constexpr (TABLE_ADD || DBL1) pair_qtab_build_odd_add29<QTab>(Qp, QX, QY, qtab, odd);
        else pair_qtab_build_odd29<QTab>(Qp, qtab, odd);
        u256 k;
        u2_fold_odd(k, u2);
        pair_u2_mult_odd29<QTab, DBL1>(T, k, qtab, odd);
        t_inf = false;
    } else {
        pair_qtab_build29<QTab, W>(Qp, QX, QY, qtab, odd);
        pair_u2_mult29<QTab, W, DBL1>(T, t_inf, u2, Qp, qtab, odd);
    }

    // --- S = u1 * G (16-bit comb), then R = S + T ---
    pair_pt S;
    bool s_inf;
    pair_comb_mult29<GTab16>(S, s_inf, u1, gtab, Qp, odd);
    pair_final_add29(Rr, r_inf, S, s_inf, T, t_inf, odd);
}

// R = u1*G + u2*Q with both points on comb tables (registered key): 16 + 32 pair mixed additions.
template <class KTab = KeyTab8>
__device__ __forceinline__ void pair_combined_mult_keyed29(pair_pt& Rr, bool& r_inf, const u256& u1, const u256& u2,
                                                           const int32_t* __restrict__ gtab, const int32_t* __restrict__ ktab, bool odd) {
    const fe ONE = {FE29_R1};
    fe gx, gy;
    GTab16 gt{gtab};
    gt.load(0, 1u, gx, gy);
    pair_pt seed, S, T;
    seed.A = gx;
    fe_sel(seed.B, odd, ONE, gy);
    bool s_inf, t_inf;
    pair_comb_mult29<KTab>(T, t_inf, u2, ktab, seed, odd);
    pair_comb_mult29<GTab16>(S, s_inf, u1, gtab, seed, odd);
    pair_final_add29(Rr, r_inf, S, s_inf, T, t_inf, odd);
}

// x(R) mod n == r on a pair: Z^2 and r Z^2 on O, the comparison with X on E.  The result is valid on the EVEN lane.
// NB the swapped operand is the MINUEND: hipcc folds the DPP move into the subtraction, and for "own - partner" it emits
// v_subrev_u32_dpp, which on MI355X does not compute src1 - dpp(src0) (probed in gputest.hip op 3; the Makefile rejects
// any build whose device code contains that opcode).
__device__ __forceinline__ bool pair_x_equals_r29(const pair_pt& Rr, bool r_inf, const u256& r) {
    const u256 N = FAB_P256_N;
    const u256 PMN = FAB_P256_P_MINUS_N;
    fe zz, rm, rhs, rhs_e, d;
    u256 r2;
    fe_sqr(zz, Rr.B);                                  // O: Z^2
    fe_to_mont(rm, r);
    fe_mul(rhs, rm, zz);
    pair_swap_fe(rhs_e, rhs);                          // E: r Z^2
    fe_sub(d, rhs_e, Rr.A);
    bool ok = fe_is_zero(d);
    add256(r2, r, N);
    fe_to_mont(rm, r2);
    fe_mul(rhs, rm, zz);
    pair_swap_fe(rhs_e, rhs);
    fe_sub(d, rhs_e, Rr.A);
    ok = ok | (lt256(r, PMN) & fe_is_zero(d));
    return ok & !r_inf;
}

// Status of one tuple, valid on the EVEN lane of the pair.
template <class QTab, int W = 5, bool DBL1 = false, bool BOOTH4 = false, bool TABLE_ADD = false>
__device__ __forceinline__ uint32_t p256_verify_pair29(const u256& qx, const u256& qy, const u256& e, const u256& r, const u256& s,
                                                        const int32_t* __restrict__ gtab, const QTab& qtab, bool odd) {
    const u256 P = FAB_P256_P;
    uint32_t early = range_status(r, s);

    bool q_in_field = lt256(qx, P) & lt256(qy, P);
    fe QX, QY;
    fe_to_mont(QX, qx);
    fe_to_mont(QY, qy);
    bool q_ok = q_in_field & on_curve29(QX, QY);
    if (early == ST_VALID && !q_ok) early = ST_OFF_CURVE;

    u256 u1, u2;
    pair_ecdsa_scalars29(u1, u2, e, r, s, odd);

    pair_pt Rr;
    bool r_inf;
    pair_combined_mult29<QTab, W, DBL1, BOOTH4, TABLE_ADD>(Rr, r_inf, u1, u2, QX, QY, gtab, qtab, odd);
    bool ok = pair_x_equals_r29(Rr, r_inf, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    return early != ST_VALID ? early : st;
}

// Registered key (p256_verify_keyed_core29): status valid on the EVEN lane.
// ktab16: the key's 16-bit comb (round 6: FABGPU_FLAG_KEY_TABLES_16BIT; nullptr while the key has none) - a wavefront all of whose keys
// have one does 16 mixed additions for u2*Q instead of 32.
__device__ __forceinline__ uint32_t p256_verify_keyed_pair29(const u256& e, const u256& r, const u256& s, const int32_t* __restrict__ gtab,
                                                              const int32_t* __restrict__ ktab, const int32_t* __restrict__ ktab16, bool odd) {
    uint32_t early = range_status(r, s);
    u256 u1, u2;
    pair_ecdsa_scalars29(u1, u2, e, r, s, odd);
    pair_pt Rr;
    bool r_inf;
    if (__all(ktab16 != nullptr)) pair_combined_mult_keyed29<GTab16>(Rr, r_inf, u1, u2, gtab, ktab16, odd);
    else pair_combined_mult_keyed29<KeyTab8>(Rr, r_inf, u1, u2, gtab, ktab, odd);
    bool ok = pair_x_equals_r29(Rr, r_inf, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    return early != ST_VALID ? early : st;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// HELPER-WAVE FORM of the LDS-table pair kernel (p256_verify_pair_lds_kernel: 512 threads, two waves per SIMD).  The 252 doublings of
// u2*Q are one serial chain; the inversion s^-1 mod n, u1 and u2, and u1*G on the 16-bit comb do not depend on it.  A workgroup
// therefore runs two roles over the same 128 signatures: MAIN waves (threads 0..255) gate Q, build the 8-entry LDS table, run the
// 63 windows and the final addition and check; HELPER waves (threads 256..511, lane t + 256 serves the same signature and the same
// lane-pair parity as main lane t) do the scalar part and u1*G beside them, in the issue slots a lone wave per SIMD leaves idle.
// Per tile (A, B: workgroup barriers):
//     helper:  range gates, s^-1, u1, u2 -> u2 to LDS           | A |  u1*G -> S, s_inf, gate status to LDS | B |
//     main:    Q gates, table j*Q                               | A |  u2 from LDS, T = u2*Q               | B |  S from LDS, R = S + T, x(R) == r
// The two handoff regions are disjoint: the helper writes the next tile's u2 after B, when main has read this tile's; it writes the next
// tile's S after the next A, when main has read this tile's.  Two barriers per tile suffice.
// Layout after the 128 tables: word w of lane t (0..255) at word w * 256 + t (consecutive lanes, consecutive banks).
constexpr int PAIR_HAND_U2_WORDS = 8;                   // u2
constexpr int PAIR_HAND_S_WORDS = 9 + 9 + 1;            // S.A, S.B, s_inf | gate status << 1
constexpr int PAIR_HAND_WORDS = PAIR_HAND_U2_WORDS + PAIR_HAND_S_WORDS;

template <int LANES>
struct PairHandoffLds {
    uint32_t* u2;   // (LDS) this lane's first u2 word
    uint32_t* s;    // (LDS) this lane's first S word
    static __device__ __forceinline__ PairHandoffLds of(uint32_t* base, uint32_t lane) {
        return PairHandoffLds{base + lane, base + PAIR_HAND_U2_WORDS * LANES + lane};
    }
    __device__ __forceinline__ void put_u2(const u256& v) const {
#pragma unroll
        for (int w = 0; w < 8; w++) u2[w * LANES] = v.w[w];
    }
    __device__ __forceinline__ void get_u2(u256& v) const {
#pragma unroll
        for (int w = 0; w < 8; w++) v.w[w] = u2[w * LANES];
    }
    __device__ __forceinline__ void put_s(const pair_pt& S, bool s_inf, uint32_t early) const {
#pragma unroll
        for (int l = 0; l < 9; l++) s[l * LANES] = (uint32_t)S.A.v[l];
#pragma unroll
        for (int l = 0; l < 9; l++) s[(9 + l) * LANES] = (uint32_t)S.B.v[l];
        s[18 * LANES] = (s_inf ? 1u : 0u) | (early << 1);
    }
    __device__ __forceinline__ void get_s(pair_pt& S, bool& s_inf, uint32_t& early) const {
#pragma unroll
        for (int l = 0; l < 9; l++) S.A.v[l] = (int32_t)s[l * LANES];
#pragma unroll
        for (int l = 0; l < 9; l++) S.B.v[l] = (int32_t)s[(9 + l) * LANES];
        uint32_t f = s[18 * LANES];
        s_inf = (f & 1u) != 0;
        early = f >> 1;
    }
};

// Helper, before barrier A: range gates, w = s^-1 and u2 = r w; u2 goes to LDS - folded to its odd representative (u2_fold_odd: one
// subtraction and a select, off the chain; the sign rides in bit 0, the handoff stays eight words) unless BOOTH4 - w and the gate status
// stay.  u1 = e w is not wanted before the comb: pair_helper_comb29 computes it behind the barrier (round 10).
template <class Hand, bool BOOTH4 = false>
__device__ __forceinline__ void pair_helper_scalars29(u256& w, uint32_t& early, const u256& r, const u256& s, const Hand& hand, bool odd) {
    early = range_status(r, s);
    u256 u2;
    pair_ecdsa_u2_29(w, u2, r, s, odd);
    if constexpr (!BOOTH4) {
        u256 k;
        u2_fold_odd(k, u2);
        u2 = k;
    }
    hand.put_u2(u2);
}

// Helper, between A and B: u1 = e w, then S = u1*G on the 16-bit comb (seeded with G: the seed is any valid point, and this role has
// no Q), to LDS.
template <class Hand>
__device__ __forceinline__ void pair_helper_comb29(const u256& e, const u256& w, uint32_t early, const int32_t* __restrict__ gtab, const Hand& hand,
                                                   bool odd) {
    const fe ONE = {FE29_R1};
    u256 u1;
    pair_ecdsa_u1_29(u1, e, w);
    fe gx, gy;
    GTab16 gt{gtab};
    gt.load(0, 1u, gx, gy);
    pair_pt seed, S;
    seed.A = gx;
    fe_sel(seed.B, odd, ONE, gy);
    bool s_inf;
    pair_comb_mult29<GTab16>(S, s_inf, u1, gtab, seed, odd);
    hand.put_s(S, s_inf, early);
}

// Main, before barrier A: Q gates and the table (odd multiples - by co-Z additions, or by general ones for TABLE_ADD - or j*Q for BOOTH4).
// Returns q_ok; Qp = Q in pair state.
template <class QTab, bool BOOTH4 = false, bool TABLE_ADD = false>
__device__ __forceinline__ bool pair_main_table29(pair_pt& Qp, const u256& qx, const u256& qy, const QTab& qtab, bool odd) {
    const u256 P = FAB_P256_P;
    const fe ONE = {FE29_R1};
    bool q_in_field = lt256(qx, P) & lt256(qy, P);
    fe QX, QY;
    fe_to_mont(QX, qx);
    fe_to_mont(QY, qy);
    bool q_ok = q_in_field & on_curve29(QX, QY);
    Qp.A = QX;
    fe_sel(Qp.B, odd, ONE, QY);
    if constexpr (BOOTH4) pair_qtab_build29<QTab, 4>(Qp, QX, QY, qtab, odd);
    else if constexpr (TABLE_ADD) pair_qtab_build_odd_add29<QTab>(Qp, QX, QY, qtab, odd);
    else pair_qtab_build_odd29<QTab>(Qp, qtab, odd);
    return q_ok;
}

// Main, after barrier B: R = S + T, x(R) == r, and the status (valid on the EVEN lane) exactly as p256_verify_pair29 combines it.
template <class Hand>
__device__ __forceinline__ uint32_t pair_main_finish29(const pair_pt& T, bool t_inf, bool q_ok, const u256& r, const Hand& hand, bool odd) {
    pair_pt S, Rr;
    bool s_inf, r_inf;
    uint32_t early;
    hand.get_s(S, s_inf, early);
    if (early == ST_VALID && !q_ok) early = ST_OFF_CURVE;
    pair_final_add29(Rr, r_inf, S, s_inf, T, t_inf, odd);
    bool ok = pair_x_equals_r29(Rr, r_inf, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    return early != ST_VALID ? early : st;
}

}  // namespace fab
