// GPU-SIDE TEST HOOKS - built into libfabgpu_gputest.so, never into the product library.  Two kinds:
//   * single generated instruction streams (pair29_gcn.h) on one wavefront, so that tests/test_gpu_parity.py can compare every
//     output register with the reference interpreter of gcn_dsl.py;
//   * the device compilation of the product headers one primitive at a time (field, scalar, inversion, point and scalar-loop code)
//     over grids of many wavefronts, for tests/test_device_primitives.py to compare with big integers ("primitives on many
//     wavefronts", below), and the same for the full-word P-384 code of p384.h, p384_dev.h, p384_tables.h, p384_tables16.h and
//     p384_wide.h, for tests/test_p384_device_primitives.py ("P-384 primitives on many wavefronts", at the end).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "p256_pair29.h"
#include "pair29_bn_gcn.h"   // the BN pair programs of bn_quad29.h: validated here register for register
#include "p256_tables29.h"
#include "bn_nym29.h"
#include "bn_quad29.h"
#include "bn_tables29.h"
#include "device_common.h"
#include "p384_dev.h"        // p384.h and the row loads of the P-384 kernels
#include "p384_tables16.h"   // p384_tables.h and the 16-bit comb's digit accessor
#include "p384_wide.h"

using namespace fab;

// in : per lane A[9] B[9] C[9] D[9];  out: per lane A[9] B[9] H[9] RR[9]
__global__ void __launch_bounds__(64, 1) gputest_pair_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
    const int32_t* p = in + threadIdx.x * 36;
    pair_pt P;
    fe C, D;
    for (int i = 0; i < 9; i++) {
        P.A.v[i] = p[i];
        P.B.v[i] = p[9 + i];
        C.v[i] = p[18 + i];
        D.v[i] = p[27 + i];
    }
    PAIR_TMPS;
    for (int i = 0; i < 9; i++) tH.v[i] = tRR.v[i] = 0;
    if (op == 3) {   // ISA probe: out A = v_subrev_u32_dpp(A, B), out B = v_sub_u32_dpp(A, B), out H = v_add_u32_dpp(A, B), out RR = v_mov_b32_dpp(A)
        fe a = P.A, b = P.B;
        for (int i = 0; i < 9; i++) {
            asm volatile("s_nop 4\n\tv_subrev_u32_dpp %0, %4, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                         "v_sub_u32_dpp %1, %4, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                         "v_add_u32_dpp %2, %4, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                         "v_mov_b32_dpp %3, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 4"
                         : "=&v"(P.A.v[i]), "=&v"(P.B.v[i]), "=&v"(tH.v[i]), "=&v"(tRR.v[i])
                         : "v"(a.v[i]), "v"(b.v[i]));
        }
    } else if (op == 0) {
        PAIR_DBL(P);
    } else if (op == 1) {
        pair_pt R;
        PAIR_ADD(R, P, C, D);
        P = R;
    } else if (op == 2) {
        pair_pt R;
        PAIR_MADD(R, P, C, D);
        P = R;
    } else if (op == 7) {           // the four doublings of a 4-bit window as one program (round 8)
        PAIR_DBL4(P);
    } else if (op == 8) {           // the co-Z table build's doubling with update (round 10): out H, RR = the point over the double's Z
        PAIR_DBLU(P, tH, tRR);
    } else if (op == 9) {           // ... and its co-Z addition with update: in C, D = the other point's X, Y; out H, RR = its update
        pair_pt R;
        fe nx, ny;
        PAIR_ZADDU(R, nx, ny, P, C, D);
        P = R;
        tH = nx;
        tRR = ny;
    } else if (op == 4) {           // the same three programs for FP256BN's field and a = 0 (pair29_bn_gcn.h)
        PAIRBN_DBL(P.A, P.B, tU1, tU2, tU3, tU4, tP1, tP2, tT0, tT1, tTD);
    } else if (op == 5) {
        pair_pt R;
        PAIRBN_ADD(R.A, R.B, P.A, P.B, tH, tRR, tW, tU1, tU2, tU3, tU4, tU6, tP1, tP2, tT0, tT1, tTD, C, D);
        P = R;
    } else {
        pair_pt R;
        PAIRBN_MADD(R.A, R.B, P.A, P.B, tU1, tU2, tU3, tU4, tH, tRR, tP1, tP2, tT0, tT1, tTD, C, D);
        P = R;
    }
    int32_t* o = out + threadIdx.x * 36;
    for (int i = 0; i < 9; i++) {
        o[i] = P.A.v[i];
        o[9 + i] = P.B.v[i];
        o[18 + i] = tH.v[i];
        o[27 + i] = tRR.v[i];
    }
}

extern "C" int gputest_pair_op(int op, const int32_t* in, int32_t* out) {
    int32_t *din = nullptr, *dout = nullptr;
    const size_t bytes = 64 * 36 * sizeof(int32_t);
    if (hipMalloc((void**)&din, bytes) != hipSuccess || hipMalloc((void**)&dout, bytes) != hipSuccess) return -1;
    hipMemcpy(din, in, bytes, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(gputest_pair_kernel, dim3(1), dim3(64), 0, 0, op, din, dout);
    int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
    hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    hipFree(din);
    hipFree(dout);
    return rc;
}

// R = u1*G + u2*Q through pair_combined_mult29 on one wavefront (32 signatures).  in: 32 x (u1, u2, qx, qy) big-endian 32-byte
// fields;  out: per lane A[9] B[9] r_inf
__global__ void __launch_bounds__(64, 1) gputest_pair_combined_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ gtab,
                                                                       uint4* __restrict__ qws, int32_t* __restrict__ out) {
    const bool odd = (threadIdx.x & 1) != 0;
    const uint32_t k = threadIdx.x >> 1;
    u256 u1, u2, qx, qy;
    from_be32(u1, in + 128 * k);
    from_be32(u2, in + 128 * k + 32);
    from_be32(qx, in + 128 * k + 64);
    from_be32(qy, in + 128 * k + 96);
    fe QX, QY;
    fe_to_mont(QX, qx);
    fe_to_mont(QY, qy);
    PairQTab<32> qtab = PairQTab<32>::of(qws, k);
    pair_pt R;
    bool inf;
    pair_combined_mult29(R, inf, u1, u2, QX, QY, gtab, qtab, odd);
    int32_t* o = out + threadIdx.x * 19;
    for (int i = 0; i < 9; i++) {
        o[i] = R.A.v[i];
        o[9 + i] = R.B.v[i];
    }
    o[18] = inf ? 1 : 0;
}

extern "C" int gputest_pair_combined(const uint8_t* in, int32_t* out) {
    std::vector<int32_t> tab(GTab16::TABLE_WORDS);
    build_g_comb_table16(tab.data());
    uint8_t* din = nullptr;
    int32_t *dtab = nullptr, *dout = nullptr;
    uint4* dws = nullptr;
    if (hipMalloc((void**)&din, 32 * 128) != hipSuccess || hipMalloc((void**)&dtab, sizeof(int32_t) * GTab16::TABLE_WORDS) != hipSuccess ||
        hipMalloc((void**)&dout, 64 * 19 * 4) != hipSuccess || hipMalloc((void**)&dws, (size_t)16 * 8 * 32 * 16) != hipSuccess)
        return -1;
    hipMemcpy(din, in, 32 * 128, hipMemcpyHostToDevice);
    hipMemcpy(dtab, tab.data(), sizeof(int32_t) * GTab16::TABLE_WORDS, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(gputest_pair_combined_kernel, dim3(1), dim3(64), 0, 0, din, dtab, dws, dout);
    int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
    hipMemcpy(out, dout, 64 * 19 * 4, hipMemcpyDeviceToHost);
    hipFree(din); hipFree(dtab); hipFree(dout); hipFree(dws);
    return rc;
}

// Debug probe of p256_verify_pair29: same statements, intermediate values written out.
// in: 32 x (qx, qy, e, r, s);  out per lane: u1[8] u2[8] A[9] B[9] flags(st, ok1, ok2, r_inf, early)
__global__ void __launch_bounds__(64, 1) gputest_pair_verify_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ gtab,
                                                                     uint4* __restrict__ qws, int32_t* __restrict__ out) {
    const bool odd = (threadIdx.x & 1) != 0;
    const uint32_t k = threadIdx.x >> 1;
    u256 qx, qy, e, r, s;
    from_be32(qx, in + 160 * k);
    from_be32(qy, in + 160 * k + 32);
    from_be32(e, in + 160 * k + 64);
    from_be32(r, in + 160 * k + 96);
    from_be32(s, in + 160 * k + 128);
    PairQTab<32> qtab = PairQTab<32>::of(qws, k);
    const u256 P = FAB_P256_P;
    const u256 N = FAB_P256_N;
    uint32_t early = range_status(r, s);
    bool q_in_field = lt256(qx, P) & lt256(qy, P);
    fe QX, QY;
    fe_to_mont(QX, qx);
    fe_to_mont(QY, qy);
    bool q_ok = q_in_field & on_curve29(QX, QY);
    if (early == ST_VALID && !q_ok) early = ST_OFF_CURVE;
    u256 w, u1, u2, ered, t;
    {
        const modinv_info NI = MODINV_N_INFO;
        modinv(w, s, NI);
    }
    uint32_t br = sub256(t, e, N);
    sel256(ered, br == 0, t, e);
    fn_to_mont(t, ered);
    fn_mul(u1, t, w);
    fn_to_mont(t, r);
    fn_mul(u2, t, w);
    pair_pt Rr;
    bool r_inf;
    pair_combined_mult29(Rr, r_inf, u1, u2, QX, QY, gtab, qtab, odd);
    fe zz, rm, rhs, rhs_e, d;
    fe_sqr(zz, Rr.B);
    fe_to_mont(rm, r);
    fe_mul(rhs, rm, zz);
    pair_swap_fe(rhs_e, rhs);
    fe_sub(d, Rr.A, rhs_e);
    bool ok1 = fe_is_zero(d);
    uint32_t st = p256_verify_pair29(qx, qy, e, r, s, gtab, qtab, odd);
    int32_t* o = out + threadIdx.x * 48;
    for (int i = 0; i < 8; i++) {
        o[i] = (int32_t)u1.w[i];
        o[8 + i] = (int32_t)u2.w[i];
    }
    for (int i = 0; i < 9; i++) {
        o[16 + i] = Rr.A.v[i];
        o[25 + i] = Rr.B.v[i];
    }
    o[34] = (int32_t)st;
    o[35] = ok1;
    o[36] = r_inf;
    o[37] = (int32_t)early;
    for (int i = 0; i < 9; i++) o[38 + i] = rhs_e.v[i];
}

extern "C" int gputest_pair_verify(const uint8_t* in, int32_t* out) {
    std::vector<int32_t> tab(GTab16::TABLE_WORDS);
    build_g_comb_table16(tab.data());
    uint8_t* din = nullptr;
    int32_t *dtab = nullptr, *dout = nullptr;
    uint4* dws = nullptr;
    if (hipMalloc((void**)&din, 32 * 160) != hipSuccess || hipMalloc((void**)&dtab, sizeof(int32_t) * GTab16::TABLE_WORDS) != hipSuccess ||
        hipMalloc((void**)&dout, 64 * 48 * 4) != hipSuccess || hipMalloc((void**)&dws, (size_t)16 * 8 * 32 * 16) != hipSuccess)
        return -1;
    hipMemcpy(din, in, 32 * 160, hipMemcpyHostToDevice);
    hipMemcpy(dtab, tab.data(), sizeof(int32_t) * GTab16::TABLE_WORDS, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(gputest_pair_verify_kernel, dim3(1), dim3(64), 0, 0, din, dtab, dws, dout);
    int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
    hipMemcpy(out, dout, 64 * 48 * 4, hipMemcpyDeviceToHost);
    hipFree(din); hipFree(dtab); hipFree(dout); hipFree(dws);
    return rc;
}

// The commitment t of the pseudonym-signature equation as the DEVICE computes it (bn_nym29.h), exposed on its own so that tests can
// compare it with vectors made by an independent implementation (tests/golden/idemix_nym_kats.json): one wave, up to 64 signatures
// with one lane each (split == 0), 32 with two lanes each (split == 1) or 16 with four lanes each (split == 2).  in: n x 5 big-endian fields (nym_x, nym_y, c, s_sk, s_rnym);
// out: n x (tx[32] ty[32]) big-endian, st: n status words.
__global__ void __launch_bounds__(64, 1) gputest_nym_commitment_kernel(int split, uint32_t n, const uint8_t* __restrict__ in, const int32_t* __restrict__ hskt,
                                                                        const int32_t* __restrict__ hrandt, uint4* __restrict__ qws, uint8_t* __restrict__ out,
                                                                        uint32_t* __restrict__ st_out) {
    GlobalQTab29<64> qtab = GlobalQTab29<64>::of(qws, threadIdx.x);
    KeyTab8 hsk{hskt}, hrand{hrandt};
    const bool odd = (threadIdx.x & 1u) != 0;
    uint32_t i = split == 2 ? threadIdx.x >> 2 : (split ? threadIdx.x >> 1 : threadIdx.x);
    bool active = i < n;
    uint32_t ic = active ? i : n - 1;
    u256 nx, ny, c, ssk, srn, tx, ty;
    from_be32(nx, in + 160 * ic);
    from_be32(ny, in + 160 * ic + 32);
    from_be32(c, in + 160 * ic + 64);
    from_be32(ssk, in + 160 * ic + 96);
    from_be32(srn, in + 160 * ic + 128);
    uint32_t st;
    if (split == 2) {            // four lanes per signature (bn_quad29.h): 16 signatures on the wave, lane 4k reports
        PairBNQTab pq = PairBNQTab::of(qws, threadIdx.x >> 1);
        bn_nym_quad_half mine;
        bn_nym_quad_part1(mine, odd, (threadIdx.x & 2u) != 0, nx, ny, c, ssk, srn, hskt, hrandt, pq);
        st = bn_nym_quad_part2(tx, ty, mine, odd);
        if (active && (threadIdx.x & 3u) == 0) {
            to_be32(out + 64 * i, tx);
            to_be32(out + 64 * i + 32, ty);
            st_out[i] = st;
        }
        return;
    }
    if (!split) {
        st = bn_nym_commitment29(tx, ty, nx, ny, c, ssk, srn, hsk, hrand, qtab);
    } else {
        bn_nym_half mine;
        bn_nym_split_part1(mine, odd, nx, ny, c, ssk, srn, hsk, hrand, qtab);
        jacbn theirs;
        for (int l = 0; l < 9; l++) {
            theirs.X.v[l] = lane_pair_swap(mine.P.X.v[l]);
            theirs.Y.v[l] = lane_pair_swap(mine.P.Y.v[l]);
            theirs.Z.v[l] = lane_pair_swap(mine.P.Z.v[l]);
        }
        bool theirs_inf = lane_pair_swap(mine.inf ? 1 : 0) != 0;
        st = bn_nym_split_part2(tx, ty, mine, theirs, theirs_inf);
    }
    if (active && (!split || !odd)) {
        to_be32(out + 64 * i, tx);
        to_be32(out + 64 * i + 32, ty);
        st_out[i] = st;
    }
}

extern "C" int gputest_nym_commitment(int split, uint32_t n, const uint8_t* hsk_xy64, const uint8_t* hrand_xy64, const uint8_t* in, uint8_t* out, uint32_t* st) {
    if (n == 0 || n > (split == 2 ? 16u : (split ? 32u : 64u))) return -3;
    std::vector<int32_t> t1(KeyTab8::TABLE_WORDS), t2(KeyTab8::TABLE_WORDS);
    u256 x, y;
    from_be32(x, hsk_xy64); from_be32(y, hsk_xy64 + 32);
    build_bn_comb_table8(t1.data(), x, y);
    from_be32(x, hrand_xy64); from_be32(y, hrand_xy64 + 32);
    build_bn_comb_table8(t2.data(), x, y);
    const size_t tb = sizeof(int32_t) * KeyTab8::TABLE_WORDS;
    int32_t *d1 = nullptr, *d2 = nullptr;
    uint8_t *din = nullptr, *dout = nullptr;
    uint32_t* dst = nullptr;
    uint4* dws = nullptr;
    if (hipMalloc((void**)&d1, tb) != hipSuccess || hipMalloc((void**)&d2, tb) != hipSuccess || hipMalloc((void**)&din, 160 * n) != hipSuccess ||
        hipMalloc((void**)&dout, 64 * n) != hipSuccess || hipMalloc((void**)&dst, 4 * n) != hipSuccess ||
        hipMalloc((void**)&dws, (size_t)16 * 8 * 64 * 16) != hipSuccess)
        return -1;
    hipMemcpy(d1, t1.data(), tb, hipMemcpyHostToDevice);
    hipMemcpy(d2, t2.data(), tb, hipMemcpyHostToDevice);
    hipMemcpy(din, in, 160 * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(gputest_nym_commitment_kernel, dim3(1), dim3(64), 0, 0, split, n, din, d1, d2, dws, dout, dst);
    int rc = hipDeviceSynchronize() == hipSuccess ? 0 : -2;
    hipMemcpy(out, dout, 64 * n, hipMemcpyDeviceToHost);
    hipMemcpy(st, dst, 4 * n, hipMemcpyDeviceToHost);
    hipFree(d1); hipFree(d2); hipFree(din); hipFree(dout); hipFree(dst); hipFree(dws);
    return rc;
}

// ---- the integer multiply-accumulate ceiling of this chip, SUSTAINED ---------------------------------------------------------------
// What roofline.frac of the verify kernels is priced against (bench.py): every SIMD of the chip issuing nothing but independent
// v_mad_i64_i32 - the instruction the field products are made of - for several milliseconds, at 1, 2 or 4 wavefronts per SIMD.  Short
// bursts (ubench.hip: 40-130 us) run at the boost clock; a kernel that keeps the multiplier array busy for milliseconds runs at
// whatever clock the power budget leaves, and that is the ceiling a 0.7 ms verify launch actually lives under.
// Reports wall time (HIP events), the shader-clock ticks one wavefront counted (s_memtime) and the MACs retired.
__global__ void __launch_bounds__(1024) gputest_mac_ceiling_kernel(uint32_t iters, uint32_t seed, uint64_t* __restrict__ ticks) {
    int32_t a = (int32_t)(seed + threadIdx.x), b = (int32_t)(seed * 3 + 1);
    int64_t x0 = a, x1 = b, x2 = a ^ 77, x3 = threadIdx.x, x4 = a + 1, x5 = b + 2, x6 = a + 3, x7 = b + 4;
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    for (uint32_t it = 0; it < iters; it++) {
#define MAC8 "v_mad_i64_i32 %0, s[10:11], %8, %9, %0\n v_mad_i64_i32 %1, s[10:11], %8, %9, %1\n v_mad_i64_i32 %2, s[10:11], %8, %9, %2\n v_mad_i64_i32 %3, s[10:11], %8, %9, %3\n" \
             "v_mad_i64_i32 %4, s[10:11], %8, %9, %4\n v_mad_i64_i32 %5, s[10:11], %8, %9, %5\n v_mad_i64_i32 %6, s[10:11], %8, %9, %6\n v_mad_i64_i32 %7, s[10:11], %8, %9, %7\n"
        asm volatile(MAC8 MAC8 MAC8 MAC8 MAC8 MAC8 MAC8 MAC8
                     : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7)
                     : "v"(a), "v"(b)
                     : "s10", "s11");
#undef MAC8
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    const uint64_t sink = (uint64_t)(x0 ^ x1 ^ x2 ^ x3 ^ x4 ^ x5 ^ x6 ^ x7);
    if ((threadIdx.x & 63) == 0) ticks[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = (t1 - t0) + (sink == 0x1234567 ? 1 : 0);
}

// waves_per_simd in {1, 2, 4}; iters x 64 MAC instructions per wavefront.  out: [0] wall ms, [1] mean s_memtime ticks per wavefront,
// [2] MACs retired (lanes x instructions), [3] wavefronts.  0 ok.
extern "C" int gputest_mac_ceiling(int waves_per_simd, uint32_t iters, double* out4) {
    if (!out4 || (waves_per_simd != 1 && waves_per_simd != 2 && waves_per_simd != 4)) return 1;
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 2;
    const int cus = prop.multiProcessorCount, threads = 256 * waves_per_simd, waves = cus * 4 * waves_per_simd;
    uint64_t* d = nullptr;
    if (hipMalloc(&d, sizeof(uint64_t) * waves) != hipSuccess) return 3;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipLaunchKernelGGL(gputest_mac_ceiling_kernel, dim3(cus), dim3(threads), 0, 0, iters / 16 + 1, 12345u, d);     // warm-up
    hipDeviceSynchronize();
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL(gputest_mac_ceiling_kernel, dim3(cus), dim3(threads), 0, 0, iters, 12345u, d);
    hipEventRecord(e1, 0);
    int rc = hipEventSynchronize(e1) == hipSuccess ? 0 : 4;
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<uint64_t> h(waves);
    if (rc == 0 && hipMemcpy(h.data(), d, sizeof(uint64_t) * waves, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    double sum = 0;
    for (uint64_t v : h) sum += (double)v;
    out4[0] = ms;
    out4[1] = sum / waves;
    out4[2] = (double)waves * 64.0 * 64.0 * (double)iters;
    out4[3] = waves;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(d);
    return rc;
}

// ---- wave placement of a 512-thread workgroup --------------------------------------------------------------------------------------
// The helper-wave pair kernel (kernels.hip p256_verify_pair_lds_kernel) assumes that wavefront k and wavefront k + 4 of its 512-thread
// workgroup share a SIMD (main wave k and helper wave k + 4 serve the same signatures).  This probe launches workgroups of that shape
// with the same dynamic LDS (one workgroup per CU) and records the HW_ID register (a read: s_getreg_b32) of every wavefront:
// out[8 g + w] = HW_ID of wavefront w of workgroup g (bits 5:4 SIMD, 11:8 CU, 12 SH, 15:13 SE).  Placement decides speed only.
__global__ void __launch_bounds__(512, 1) gputest_wave_placement_kernel(uint32_t* __restrict__ out) {
    extern __shared__ uint32_t placement_lds[];
    const uint32_t id = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // hwreg(HW_REG_HW_ID, 0, 32)
    placement_lds[threadIdx.x] = id;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 8 + (threadIdx.x >> 6)] = placement_lds[threadIdx.x];
}

extern "C" int gputest_wave_placement(uint32_t wgs, uint32_t lds_bytes, uint32_t* out) {
    if (!out || wgs == 0 || lds_bytes < 512 * 4) return 1;
    uint32_t* d = nullptr;
    if (hipMalloc(&d, sizeof(uint32_t) * 8 * wgs) != hipSuccess) return 3;
    hipLaunchKernelGGL(gputest_wave_placement_kernel, dim3(wgs), dim3(512), lds_bytes, 0, d);
    int rc = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : 4;
    if (rc == 0 && hipMemcpy(out, d, sizeof(uint32_t) * 8 * wgs, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    hipFree(d);
    return rc;
}

// ---- primitives on many wavefronts ---------------------------------------------------------------------------------------------------
// The DEVICE compilation of the product headers, one primitive at a time, for tests/test_device_primitives.py: wherever a header
// branches on __HIP_DEVICE_COMPILE__ (the generated asm of fe29_gcn.h / bn29_gcn.h / one29_gcn.h, the mac of fp256.h, the ballots that
// end modinv and pair_modinv) the host tests run something else.  n items over a grid of 256-thread workgroups; one lane per item, or
// one lane PAIR per item for the pair primitives (every lane of the pair writes its own result).  Lanes past the end clamp to the
// last item - they take part in every ballot and DPP exchange - and write nothing.
namespace {
constexpr uint32_t PRIM_BLOCK = 256;
constexpr uint32_t PRIM_MAX_ITEMS = 1u << 22;

struct DevBufs {   // the device buffers of one hook call, released together
    std::vector<void*> held;
    ~DevBufs() {
        for (void* q : held) hipFree(q);
    }
    void* get(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
        held.push_back(q);
        return q;
    }
    void* put(const void* src, size_t bytes) {
        void* q = get(bytes);
        if (q && bytes && hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return q;
    }
};
inline dim3 prim_grid(size_t lanes) { return dim3((unsigned)((lanes + PRIM_BLOCK - 1) / PRIM_BLOCK)); }
inline int prim_sync() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -2; }
inline bool prim_back(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; }

template <class F>
__device__ __forceinline__ void prim_load_fe(F& r, const int32_t* p) {
#pragma unroll
    for (int l = 0; l < 9; l++) r.v[l] = p[l];
}
template <class F>
__device__ __forceinline__ void prim_store_fe(int32_t* p, const F& a) {
#pragma unroll
    for (int l = 0; l < 9; l++) p[l] = a.v[l];
}
}  // namespace

// Field operations of fe (P-256, fe29.h) and fbn (FP256BN, bn29.h).  form 0: a, b are 32 big-endian bytes per item, brought into the
// field on the device (fe_to_mont);  form 1: nine int32 limbs per item, used as they are.
// op: 0 a * b   1 a^2   2 (a + b) * (a - b)   3 (2a) * b   4 fe_weak_norm(a)   5 a itself (form 0: the to_mont -> from_mont round trip)
// out per item: limbs[9] of the result, canon[32] = fe_from_mont(result) big-endian, zero = fe_is_zero(result)
template <class F>
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_field_kernel(int op, int form, uint32_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                    int32_t* __restrict__ limbs, uint8_t* __restrict__ canon, uint32_t* __restrict__ zero) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    F A, B, Rr, t1, t2;
    if (form == 0) {
        u256 x, y;
        from_be32(x, a + 32 * (size_t)ic);
        from_be32(y, b + 32 * (size_t)ic);
        fe_to_mont(A, x);
        fe_to_mont(B, y);
    } else {
        prim_load_fe(A, reinterpret_cast<const int32_t*>(a) + 9 * (size_t)ic);
        prim_load_fe(B, reinterpret_cast<const int32_t*>(b) + 9 * (size_t)ic);
    }
    if (op == 0) {
        fe_mul(Rr, A, B);
    } else if (op == 1) {
        fe_sqr(Rr, A);
    } else if (op == 2) {
        fe_add(t1, A, B);
        fe_sub(t2, A, B);
        fe_mul(Rr, t1, t2);
    } else if (op == 3) {
        fe_dbl(t1, A);
        fe_mul(Rr, t1, B);
    } else if (op == 4) {
        fe_weak_norm(Rr, A);
    } else {
        Rr = A;
    }
    u256 c;
    fe_from_mont(c, Rr);
    const bool z = fe_is_zero(Rr);
    if (active) {
        prim_store_fe(limbs + 9 * (size_t)i, Rr);
        to_be32(canon + 32 * (size_t)i, c);
        zero[i] = z ? 1u : 0u;
    }
}

// field: 0 P-256, 1 FP256BN.  0 ok, -1 allocation or copy in, -2 launch or kernel, -3 arguments, -4 copy out.
extern "C" int gputest_field_op(int field, int op, int form, uint32_t n, const void* a, const void* b, int32_t* limbs, uint8_t* canon, uint32_t* zero) {
    if ((field | 1) != 1 || op < 0 || op > 5 || (form | 1) != 1 || n == 0 || n > PRIM_MAX_ITEMS || !a || !b || !limbs || !canon || !zero) return -3;
    const size_t in_bytes = (size_t)n * (form ? 36 : 32);
    DevBufs d;
    const uint8_t* da = (const uint8_t*)d.put(a, in_bytes);
    const uint8_t* db = (const uint8_t*)d.put(b, in_bytes);
    int32_t* dl = (int32_t*)d.get((size_t)n * 36);
    uint8_t* dc = (uint8_t*)d.get((size_t)n * 32);
    uint32_t* dz = (uint32_t*)d.get((size_t)n * 4);
    if (!da || !db || !dl || !dc || !dz) return -1;
    if (field == 0) hipLaunchKernelGGL(gputest_field_kernel<fe>, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, form, n, da, db, dl, dc, dz);
    else hipLaunchKernelGGL(gputest_field_kernel<fbn>, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, form, n, da, db, dl, dc, dz);
    int rc = prim_sync();
    if (rc == 0 && !(prim_back(limbs, dl, (size_t)n * 36) && prim_back(canon, dc, (size_t)n * 32) && prim_back(zero, dz, (size_t)n * 4))) rc = -4;
    return rc;
}

// The scalar field mod n and the 256-bit helpers of fp256.h / p256_point.h.  a, b, c: 32 big-endian bytes per item.
// op: 0 fn_to_mont(a)   1 fn_mul(a, b)   2 sub256(a, b): out0 = difference, flag = borrow   3 sel256(c odd, a, b)   4 flag = lt256(a, b)
//     5 flag = range_status(r = a, s = b)   6 ecdsa_scalars29(e = a, r = b, s = c): out0 = u1, out1 = u2
//     7 pair_ecdsa_scalars29, one lane pair per item
// out per LANE (ops 0..6: lane = item; op 7: lanes 2k and 2k + 1 serve item k): out0[32] out1[32] big-endian, flag
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_scalar_kernel(int op, uint32_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                     const uint8_t* __restrict__ c, uint8_t* __restrict__ out, uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const uint32_t i = op == 7 ? t >> 1 : t;
    const bool odd = op == 7 && (t & 1u) != 0;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    u256 A, B, C, o0 = zero256(), o1 = zero256();
    uint32_t f = 0;
    from_be32(A, a + 32 * (size_t)ic);
    from_be32(B, b + 32 * (size_t)ic);
    from_be32(C, c + 32 * (size_t)ic);
    if (op == 0) fn_to_mont(o0, A);
    else if (op == 1) fn_mul(o0, A, B);
    else if (op == 2) f = sub256(o0, A, B);
    else if (op == 3) sel256(o0, (C.w[0] & 1u) != 0, A, B);
    else if (op == 4) f = lt256(A, B) ? 1u : 0u;
    else if (op == 5) f = range_status(A, B);
    else if (op == 6) ecdsa_scalars29(o0, o1, A, B, C);
    else pair_ecdsa_scalars29(o0, o1, A, B, C, odd);
    if (active) {
        to_be32(out + 64 * (size_t)t, o0);
        to_be32(out + 64 * (size_t)t + 32, o1);
        flag[t] = f;
    }
}

extern "C" int gputest_scalar_op(int op, uint32_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out, uint32_t* flag) {
    if (op < 0 || op > 7 || n == 0 || n > PRIM_MAX_ITEMS || !a || !b || !c || !out || !flag) return -3;
    const size_t lanes = (size_t)n * (op == 7 ? 2 : 1);
    DevBufs d;
    const uint8_t* da = (const uint8_t*)d.put(a, (size_t)n * 32);
    const uint8_t* db = (const uint8_t*)d.put(b, (size_t)n * 32);
    const uint8_t* dc = (const uint8_t*)d.put(c, (size_t)n * 32);
    uint8_t* dout = (uint8_t*)d.get(lanes * 64);
    uint32_t* df = (uint32_t*)d.get(lanes * 4);
    if (!da || !db || !dc || !dout || !df) return -1;
    hipLaunchKernelGGL(gputest_scalar_kernel, prim_grid(lanes), dim3(PRIM_BLOCK), 0, 0, op, n, da, db, dc, dout, df);
    int rc = prim_sync();
    if (rc == 0 && !(prim_back(out, dout, lanes * 64) && prim_back(flag, df, lanes * 4))) rc = -4;
    return rc;
}

// The GLV decomposition of the pseudonym kernels (bn_nym29.h bn_glv_decompose: mul512 / sub256 chains, whose device compilation is the
// mac of fp256.h).  in: 32 big-endian bytes per item (any 256-bit value);  out per item: m1[32] m2[32] big-endian magnitudes, then one
// little-endian flag word, bit 0 = k1 negative, bit 1 = k2 negative.
constexpr uint32_t GLV_ROW_BYTES = 68;
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_bn_glv_decompose_kernel(uint32_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    u256 k, m1, m2;
    bool n1, n2;
    from_be32(k, in + 32 * (size_t)ic);
    bn_glv_decompose(m1, n1, m2, n2, k);
    if (active) {
        uint8_t* o = out + GLV_ROW_BYTES * (size_t)i;
        to_be32(o, m1);
        to_be32(o + 32, m2);
        o[64] = (uint8_t)((n1 ? 1u : 0u) | (n2 ? 2u : 0u));
        o[65] = 0;
        o[66] = 0;
        o[67] = 0;
    }
}

extern "C" int gputest_bn_glv_decompose(uint32_t n, const uint8_t* in, uint8_t* out) {
    if (n == 0 || n > PRIM_MAX_ITEMS || !in || !out) return -3;
    DevBufs d;
    const uint8_t* din = (const uint8_t*)d.put(in, (size_t)n * 32);
    uint8_t* dout = (uint8_t*)d.get((size_t)n * GLV_ROW_BYTES);
    if (!din || !dout) return -1;
    hipLaunchKernelGGL(gputest_bn_glv_decompose_kernel, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, n, din, dout);
    int rc = prim_sync();
    if (rc == 0 && !prim_back(out, dout, (size_t)n * GLV_ROW_BYTES)) rc = -4;
    return rc;
}

// Safegcd inversion (modinv30.h modinv; p256_pair29.h pair_modinv).  which: 0 mod n, 1 mod p (P-256), 2 mod the FP256BN prime (what
// bn_affine29 inverts by).  pair: one lane pair per item through pair_modinv, each lane's result written on its own.
// in: 32 big-endian bytes per item;  out: 32 per LANE.
// One instantiation per modulus: the kernels hand modinv a compile-time constant, so inv30 and the modulus limbs are immediates here too.
template <int WHICH>
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_modinv_kernel(int pair, uint32_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const uint32_t i = pair ? t >> 1 : t;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    const modinv_info NI = MODINV_N_INFO, PI = MODINV_P_INFO, BI = MODINV_BNP_INFO;
    const modinv_info& mi = WHICH == 0 ? NI : (WHICH == 1 ? PI : BI);   // WHICH is a template argument: the choice folds away
    u256 x, w;
    from_be32(x, in + 32 * (size_t)ic);
    if (pair) pair_modinv(w, x, mi, (t & 1u) != 0);
    else modinv(w, x, mi);
    if (active) to_be32(out + 32 * (size_t)t, w);
}

extern "C" int gputest_modinv(int which, int pair, uint32_t n, const uint8_t* in, uint8_t* out) {
    if (which < 0 || which > 2 || (pair | 1) != 1 || n == 0 || n > PRIM_MAX_ITEMS || !in || !out) return -3;
    const size_t lanes = (size_t)n * (pair ? 2 : 1);
    DevBufs d;
    const uint8_t* din = (const uint8_t*)d.put(in, (size_t)n * 32);
    uint8_t* dout = (uint8_t*)d.get(lanes * 32);
    if (!din || !dout) return -1;
    if (which == 0) hipLaunchKernelGGL(gputest_modinv_kernel<0>, prim_grid(lanes), dim3(PRIM_BLOCK), 0, 0, pair, n, din, dout);
    else if (which == 1) hipLaunchKernelGGL(gputest_modinv_kernel<1>, prim_grid(lanes), dim3(PRIM_BLOCK), 0, 0, pair, n, din, dout);
    else hipLaunchKernelGGL(gputest_modinv_kernel<2>, prim_grid(lanes), dim3(PRIM_BLOCK), 0, 0, pair, n, din, dout);
    int rc = prim_sync();
    if (rc == 0 && !prim_back(out, dout, lanes * 32)) rc = -4;
    return rc;
}

// The one-lane point operations as the device resolves them (p256_verify29.h: the programs of one29_gcn.h) on raw limbs.
// in per item: X1 Y1 Z1 X2 Y2 Z2 (6 x 9 int32; op 2 reads X2, Y2 as the affine addend, ops 0 and 3 read the first point only)
// op: 0 pt_dbl29   1 pt_add29   2 pt_add_mixed29   3 flag = on_curve29(X1, Y1)
// out per item: X Y Z H RR (5 x 9 int32; H, RR zero for ops 0 and 3), flag
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_point_kernel(int op, uint32_t n, const int32_t* __restrict__ in, int32_t* __restrict__ out, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    const int32_t* p = in + 54 * (size_t)ic;
    jac29 P1, P2, Rr;
    fe h, rr;
    prim_load_fe(P1.X, p); prim_load_fe(P1.Y, p + 9); prim_load_fe(P1.Z, p + 18);
    prim_load_fe(P2.X, p + 27); prim_load_fe(P2.Y, p + 36); prim_load_fe(P2.Z, p + 45);
    Rr = P1;
#pragma unroll
    for (int l = 0; l < 9; l++) h.v[l] = rr.v[l] = 0;
    uint32_t f = 0;
    if (op == 0) pt_dbl29(Rr, P1);
    else if (op == 1) pt_add29(Rr, P1, P2, h, rr);
    else if (op == 2) pt_add_mixed29(Rr, P1, P2.X, P2.Y, h, rr);
    else f = on_curve29(P1.X, P1.Y) ? 1u : 0u;
    if (active) {
        int32_t* o = out + 45 * (size_t)i;
        prim_store_fe(o, Rr.X); prim_store_fe(o + 9, Rr.Y); prim_store_fe(o + 18, Rr.Z);
        prim_store_fe(o + 27, h); prim_store_fe(o + 36, rr);
        flag[i] = f;
    }
}

extern "C" int gputest_point_op(int op, uint32_t n, const int32_t* in, int32_t* out, uint32_t* flag) {
    if (op < 0 || op > 3 || n == 0 || n > PRIM_MAX_ITEMS || !in || !out || !flag) return -3;
    DevBufs d;
    const int32_t* din = (const int32_t*)d.put(in, (size_t)n * 54 * 4);
    int32_t* dout = (int32_t*)d.get((size_t)n * 45 * 4);
    uint32_t* df = (uint32_t*)d.get((size_t)n * 4);
    if (!din || !dout || !df) return -1;
    hipLaunchKernelGGL(gputest_point_kernel, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, n, din, dout, df);
    int rc = prim_sync();
    if (rc == 0 && !(prim_back(out, dout, (size_t)n * 45 * 4) && prim_back(flag, df, (size_t)n * 4))) rc = -4;
    return rc;
}

// R = u1*G + u2*Q on ONE lane, the way the one-lane kernels compute it.  keyed == 0: p256_combined_mult29 (kernels.hip
// p256_verify_kernel: comb_mult29 over the generator table, the Booth-window chain over a per-lane table in a global workspace,
// final_add29), Q per item;  keyed == 1: p256_combined_mult_keyed29 with the 8-bit comb table of ONE key (key_xy64, big-endian x y) -
// the qx, qy columns of `in` are not read.  in per item: u1 u2 qx qy (4 x 32 big-endian);  out per item: X Y Z (3 x 9 int32), r_inf
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_combined_kernel(int keyed, uint32_t n, const uint8_t* __restrict__ in, const int32_t* __restrict__ gtab,
                                                                       const int32_t* __restrict__ ktab, uint4* __restrict__ qws, int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    GlobalQTab29<PRIM_BLOCK> qtab = GlobalQTab29<PRIM_BLOCK>::of(qws + (size_t)blockIdx.x * (16 * 8 * PRIM_BLOCK), threadIdx.x);
    GTab16 gt{gtab};
    u256 u1, u2, qx, qy;
    from_be32(u1, in + 128 * (size_t)ic);
    from_be32(u2, in + 128 * (size_t)ic + 32);
    from_be32(qx, in + 128 * (size_t)ic + 64);
    from_be32(qy, in + 128 * (size_t)ic + 96);
    jac29 Rr;
    bool inf;
    if (keyed) {
        KeyTab8 kt{ktab};
        p256_combined_mult_keyed29(Rr, inf, u1, u2, gt, kt);
    } else {
        const fe ONE = {FE29_R1};
        jac29 Q;
        fe_to_mont(Q.X, qx);
        fe_to_mont(Q.Y, qy);
        Q.Z = ONE;
        p256_combined_mult29(Rr, inf, u1, u2, Q, gt, qtab);
    }
    if (active) {
        int32_t* o = out + 28 * (size_t)i;
        prim_store_fe(o, Rr.X); prim_store_fe(o + 9, Rr.Y); prim_store_fe(o + 18, Rr.Z);
        o[27] = inf ? 1 : 0;
    }
}

extern "C" int gputest_combined(int keyed, uint32_t n, const uint8_t* key_xy64, const uint8_t* in, int32_t* out) {
    if ((keyed | 1) != 1 || n == 0 || n > 65536 || !in || !out || (keyed && !key_xy64)) return -3;
    std::vector<int32_t> tab(GTab16::TABLE_WORDS), ktab(KeyTab8::TABLE_WORDS, 0);
    build_g_comb_table16(tab.data());
    if (keyed) {
        u256 x, y;
        from_be32(x, key_xy64);
        from_be32(y, key_xy64 + 32);
        build_key_comb_table8(ktab.data(), x, y);
    }
    const dim3 grid = prim_grid(n);
    DevBufs d;
    const uint8_t* din = (const uint8_t*)d.put(in, (size_t)n * 128);
    const int32_t* dtab = (const int32_t*)d.put(tab.data(), sizeof(int32_t) * GTab16::TABLE_WORDS);
    const int32_t* dkt = (const int32_t*)d.put(ktab.data(), sizeof(int32_t) * KeyTab8::TABLE_WORDS);
    uint4* dws = (uint4*)d.get((size_t)grid.x * PRIM_BLOCK * 16 * 8 * sizeof(uint4));
    int32_t* dout = (int32_t*)d.get((size_t)n * 28 * 4);
    if (!din || !dtab || !dkt || !dws || !dout) return -1;
    hipLaunchKernelGGL(gputest_combined_kernel, grid, dim3(PRIM_BLOCK), 0, 0, keyed, n, din, dtab, dkt, dws, dout);
    int rc = prim_sync();
    if (rc == 0 && !prim_back(out, dout, (size_t)n * 28 * 4)) rc = -4;
    return rc;
}

// ---- P-384 primitives on many wavefronts ---------------------------------------------------------------------------------------------
// The DEVICE compilation of p384.h (under __HIP_DEVICE_COMPILE__ mont_mul is ONE out-of-line function taking two u384 by value, which
// pt_add calls from inside its only divergent branch), the row loads of p384_dev.h and the digit accessors of p384_tables.h,
// p384_tables16.h and p384_wide.h, one primitive at a time, for tests/test_p384_device_primitives.py to compare with Python integers.
// One lane per item over the PRIM_BLOCK grids above; lanes past the end clamp to the last item and write nothing.
//
// Field and scalar code.  FIELD: the modulus is p, else n.  a, b: 48 big-endian bytes per item, read by load_be_field48 (form 1: a is
// 32 bytes per item, read by load_e384<true>); out48: 48 big-endian bytes per item through to_be48; flag: one word per item.
// op:  0 mont_mul<FIELD>(a, b), raw (through fp_mul / fn_mul)   1 mod_add(a, b, m)   2 mod_sub(a, b, m)   3 to_mont(a)   4 from_mont(a)
//      5 a b as plain integers (to_mont both, product, from_mont)   6 a^2 likewise   7 a^-1 likewise (fp_inv / fn_inv; 0 -> 0)
//      8 fn_reduce_once(a)   9 add384(a, b), flag = carry   10 sub384(a, b), flag = borrow   11 flag = lt384(a, b)
//      12 flag = eq384(a, b)   13 flag = is_zero(a)   14 flag = range_status(r = a, s = b)   15 a itself (load, then store)
// Ops 11 .. 14 store a as out48.
template <bool FIELD>
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_p384_field_kernel(int op, int form, uint32_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                         uint8_t* __restrict__ out48, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    const p384::u384 P = FAB_P384_P, N = FAB_P384_N;
    const p384::u384& M = FIELD ? P : N;
    p384::u384 A, B, Rr, am, bm;
    if (form) load_e384<true>(A, a, ic);
    else load_e384<false>(A, a, ic);
    load_be_field48(B, b, ic);
    Rr = A;
    uint32_t f = 0;
    switch (op) {
        case 0:
            if (FIELD) p384::fp_mul(Rr, A, B);
            else p384::fn_mul(Rr, A, B);
            break;
        case 1: p384::mod_add(Rr, A, B, M); break;
        case 2: p384::mod_sub(Rr, A, B, M); break;
        case 3:
            if (FIELD) p384::fp_to_mont(Rr, A);
            else p384::fn_to_mont(Rr, A);
            break;
        case 4:
            if (FIELD) p384::fp_from_mont(Rr, A);
            else p384::fn_from_mont(Rr, A);
            break;
        case 5:
        case 6:
        case 7:
            if (FIELD) {
                p384::fp_to_mont(am, A);
                p384::fp_to_mont(bm, B);
                if (op == 5) p384::fp_mul(Rr, am, bm);
                else if (op == 6) p384::fp_sqr(Rr, am);
                else p384::fp_inv(Rr, am);
                p384::fp_from_mont(Rr, Rr);
            } else {
                p384::fn_to_mont(am, A);
                p384::fn_to_mont(bm, B);
                if (op == 5) p384::fn_mul(Rr, am, bm);
                else if (op == 6) p384::fn_mul(Rr, am, am);
                else p384::fn_inv(Rr, am);
                p384::fn_from_mont(Rr, Rr);
            }
            break;
        case 8: p384::fn_reduce_once(Rr, A); break;
        case 9: f = p384::add384(Rr, A, B); break;
        case 10: f = p384::sub384(Rr, A, B); break;
        case 11: f = p384::lt384(A, B) ? 1u : 0u; break;
        case 12: f = p384::eq384(A, B) ? 1u : 0u; break;
        case 13: f = p384::is_zero(A) ? 1u : 0u; break;
        case 14: f = p384::range_status(A, B); break;
        default: break;
    }
    if (active) {
        p384::to_be48(out48 + 48 * (size_t)i, Rr);
        flag[i] = f;
    }
}

// modulus: 1 p, 0 n.  0 ok, -1 allocation or copy in, -2 launch or kernel, -3 arguments, -4 copy out.
extern "C" int gputest_p384_field_op(int modulus, int op, int form, uint32_t n, const uint8_t* a, const uint8_t* b, uint8_t* out48, uint32_t* flag) {
    if ((modulus | 1) != 1 || op < 0 || op > 15 || (form | 1) != 1 || n == 0 || n > PRIM_MAX_ITEMS || !a || !b || !out48 || !flag) return -3;
    DevBufs d;
    const uint8_t* da = (const uint8_t*)d.put(a, (size_t)n * (form ? 32 : 48));
    const uint8_t* db = (const uint8_t*)d.put(b, (size_t)n * 48);
    uint8_t* dout = (uint8_t*)d.get((size_t)n * 48);
    uint32_t* df = (uint32_t*)d.get((size_t)n * 4);
    if (!da || !db || !dout || !df) return -1;
    if (modulus) hipLaunchKernelGGL(gputest_p384_field_kernel<true>, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, form, n, da, db, dout, df);
    else hipLaunchKernelGGL(gputest_p384_field_kernel<false>, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, form, n, da, db, dout, df);
    int rc = prim_sync();
    if (rc == 0 && !(prim_back(out48, dout, (size_t)n * 48) && prim_back(flag, df, (size_t)n * 4))) rc = -4;
    return rc;
}

// The digits of a scalar as every P-384 core takes them.  a: 48 big-endian bytes per item;  out per item, GPUTEST_P384_DIGIT_WORDS words:
//   [0, 96)     take_top_nibble, 96 calls in order (p384.h: verify_core)
//   [96, 144)   wide_digit(w), w = 0 .. 47 (p384_wide.h)
//   [144, 192)  take_low_byte, 48 calls in order (p384_tables.h: CombPtr384::take)
//   [192, 216)  take_low_half, 24 calls in order (p384_tables16.h: CombPtr384x16::take)
constexpr uint32_t GPUTEST_P384_DIGIT_WORDS = 216;
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_p384_digits_kernel(uint32_t n, const uint8_t* __restrict__ a, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    p384::u384 A, u;
    load_be_field48(A, a, ic);
    if (!active) return;                       // nothing below talks to another lane
    uint32_t* o = out + GPUTEST_P384_DIGIT_WORDS * (size_t)i;
    u = A;
    for (int k = 0; k < 96; k++) o[k] = p384::take_top_nibble(u);
    for (uint32_t w = 0; w < 48; w++) o[96 + w] = p384::wide_digit(A.w, w);
    u = A;
    for (int k = 0; k < 48; k++) o[144 + k] = p384::CombPtr384::take(u);
    u = A;
    for (int k = 0; k < 24; k++) o[192 + k] = p384::CombPtr384x16::take(u);
}

extern "C" int gputest_p384_digits(uint32_t n, const uint8_t* a, uint32_t* out) {
    if (n == 0 || n > PRIM_MAX_ITEMS || !a || !out) return -3;
    DevBufs d;
    const uint8_t* da = (const uint8_t*)d.put(a, (size_t)n * 48);
    uint32_t* dout = (uint32_t*)d.get((size_t)n * GPUTEST_P384_DIGIT_WORDS * 4);
    if (!da || !dout) return -1;
    hipLaunchKernelGGL(gputest_p384_digits_kernel, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, n, da, dout);
    int rc = prim_sync();
    if (rc == 0 && !prim_back(out, dout, (size_t)n * GPUTEST_P384_DIGIT_WORDS * 4)) rc = -4;
    return rc;
}

// The point operations on raw words.  in per item: X1 Y1 Z1 X2 Y2 Z2, twelve little-endian words each, canonical Montgomery form (the
// caller chooses Z and with it the representative);  out per item: X Y Z (36 words), flag.
// op: 0 pt_dbl(first)   1 pt_add<false>   2 pt_add<true> (Z2 is one)   3 flag = on_curve(X1, Y1)
//     4 flag = x_equals_r(first, r), r = the twelve words of the X2 slot as a plain integer.   Ops 3 and 4 store the first triple.
__global__ void __launch_bounds__(PRIM_BLOCK) gputest_p384_point_kernel(int op, uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                         uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * PRIM_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : n - 1;
    const uint32_t* p = in + 72 * (size_t)ic;
    p384::jac P1, P2, Rr;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        P1.X.w[k] = p[k]; P1.Y.w[k] = p[12 + k]; P1.Z.w[k] = p[24 + k];
        P2.X.w[k] = p[36 + k]; P2.Y.w[k] = p[48 + k]; P2.Z.w[k] = p[60 + k];
    }
    Rr = P1;
    uint32_t f = 0;
    if (op == 0) p384::pt_dbl(Rr, P1);
    else if (op == 1) p384::pt_add<false>(Rr, P1, P2);
    else if (op == 2) p384::pt_add<true>(Rr, P1, P2);
    else if (op == 3) f = p384::on_curve(P1.X, P1.Y) ? 1u : 0u;
    else f = p384::x_equals_r(P1, P2.X) ? 1u : 0u;
    if (active) {
        uint32_t* o = out + 36 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            o[k] = Rr.X.w[k]; o[12 + k] = Rr.Y.w[k]; o[24 + k] = Rr.Z.w[k];
        }
        flag[i] = f;
    }
}

extern "C" int gputest_p384_point_op(int op, uint32_t n, const uint32_t* in, uint32_t* out, uint32_t* flag) {
    if (op < 0 || op > 4 || n == 0 || n > PRIM_MAX_ITEMS || !in || !out || !flag) return -3;
    DevBufs d;
    const uint32_t* din = (const uint32_t*)d.put(in, (size_t)n * 72 * 4);
    uint32_t* dout = (uint32_t*)d.get((size_t)n * 36 * 4);
    uint32_t* df = (uint32_t*)d.get((size_t)n * 4);
    if (!din || !dout || !df) return -1;
    hipLaunchKernelGGL(gputest_p384_point_kernel, prim_grid(n), dim3(PRIM_BLOCK), 0, 0, op, n, din, dout, df);
    int rc = prim_sync();
    if (rc == 0 && !(prim_back(out, dout, (size_t)n * 36 * 4) && prim_back(flag, df, (size_t)n * 4))) rc = -4;
    return rc;
}
