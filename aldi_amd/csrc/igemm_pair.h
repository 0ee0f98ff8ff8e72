// The "pair" form of the 1x1 implicit GEMM: a 1x1 conv whose residual is ANOTHER 1x1 conv of a second input, both formed by one workgroup.
// Included by igemm.hip (ConvDev / PairPre, the tile primitives, igemm_epilogue_direct).
//
//   y = act( conv(x, w) * scale + shift + bf16( conv(x2, w2) * scale2 + shift2 ) )
//
// A stage's first bottleneck (res3.0 .. res5.0) ends in exactly this: conv3 of the block adds the projection shortcut of the block's input.  As
// two launches the shortcut's [N][Ho][Wo][Cout] map is written, read back once a few microseconds later and never touched again; the data
// gradient of a stage's input is the same shape of sum (conv1's dgrad + the shortcut's dgrad).  Here the 128 x 64 direct-epilogue tile
// (BF16_TAP_128x64_DR) runs ONE K loop over S1 + S2 slabs: the first S1 come from (x2, w2), the others from (x, w) -- the LDS ring, the counted
// waits and the fragment double buffering never notice the seam.  Behind the MFMAs of slab S1 - 1 the accumulators hold the inner conv; they are
// scaled, shifted and rounded to bf16 exactly as a launch of its own would have stored them, packed into the 16 registers per lane in which the DR
// tile keeps its prefetched residual (direct_perm makes the two layouts the same), and cleared.  The main conv then finishes with the unchanged
// direct epilogue.  No accumulator beyond the DR tile's, no scratch, 512 bytes more LDS (scale2 / shift2): four workgroups per CU as before.
// TWO: how the outer sum is rounded (igemm_epilogue_direct) -- a compile-time variant, as is the whole kernel: nothing here is a run-time branch of
// igemm_kernel.  K order per output element: ascending 32-channel slabs in both convs, as in every tap-form tile and the weight-stationary kernel.
#pragma once

template <bool TWO>
__global__ __launch_bounds__(256, 4) void igemm_pair_kernel(ConvDev p, PairPre q) {
    typedef bf16_t T;
    constexpr int BM = 128, BN = 64, WM = 4, WN = 1, KC = 4, NT = 256, EP = 8, BK = KC * EP;
    constexpr int A_IT = BM * KC / NT, TM = BM / WM / 16, TN = BN / WN / 16, H = TN / 2;
    static_assert(BN * KC == NT && A_IT == 2, "one weight chunk and two pixel chunks per thread and slab");
    constexpr int NBUF = 3, SLOTS = (BM + BN) * KC;
    constexpr int AUX_SLOTS = 64, AUX2_SLOTS = 32;              // [ring | scale, shift (direct epilogue's aux region) | scale2, shift2]
    __shared__ __attribute__((aligned(128))) uint4 lds_all[NBUF * SLOTS + AUX_SLOTS + AUX2_SLOTS];
    uint4 (*const lds)[SLOTS] = reinterpret_cast<uint4 (*)[SLOTS]>(&lds_all[0]);
    uint4* const aux_lds = &lds_all[NBUF * SLOTS];
    uint4* const aux2_lds = &lds_all[NBUF * SLOTS + AUX_SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave;
    const int nmt = (int)gridDim.x, nnt = (int)gridDim.y;
    int bid = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    if (p.xcd) {                                                // XCD-aware tile order, as igemm_body
        const int total = nmt * nnt, qq = total >> 3, r = total & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + idx;
    }
    const int m0 = (bid / nnt) * BM, n0 = (bid % nnt) * BN;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.x2), 0, q.x2_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.w2), 0, q.w2_bytes, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);

    // per-thread DMA sources of slab 0 of either conv; a slab's are the previous slab's + one slab of bytes (an out-of-range offset stays out of
    // range).  Both convs are 1x1 without padding: the inner one reads pixel (ho * stride2, wo * stride2) of its map, the main one pixel m.
    unsigned a1[A_IT], a2[A_IT], b1, b2;
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int c = tid + it * NT, row = c >> 2, kce = swz<KC>(row, c & (KC - 1)), m = m0 + row;
        const bool ok = m < p.M;
        const int mm = ok ? m : 0;
        const int n = mm / (p.Ho * p.Wo), r = mm - n * (p.Ho * p.Wo), ho = r / p.Wo, wo = r - ho * p.Wo;
        const unsigned pix = (unsigned)((n * q.H2 + ho * q.stride2) * q.W2 + wo * q.stride2);
        a1[it] = ok ? (pix * (unsigned)q.Cin2 + (unsigned)(kce * EP)) * 2u : OOB;
        a2[it] = ok ? ((unsigned)m * (unsigned)p.Cin + (unsigned)(kce * EP)) * 2u : OOB;
    }
    {
        const int row = tid >> 2, kce = swz<KC>(row, tid & (KC - 1));
        const int co = n0 + direct_perm<BN / WN>(row);          // (< Cout: whole 64-channel tiles)
        b1 = ((unsigned)co * (unsigned)q.Cin2 + (unsigned)(kce * EP)) * 2u;
        b2 = ((unsigned)co * (unsigned)p.K + (unsigned)(kce * EP)) * 2u;
    }
    const int S1 = q.Cin2 / BK, S = S1 + p.K / BK;              // slabs of the inner conv; of both
    auto issue_slab = [&](int s, int buf) {
        if (s < S1) {                                           // (block uniform)
#pragma unroll
            for (int it = 0; it < A_IT; ++it) {
                glds16(rx2, &lds[buf][wbase + it * NT], a1[it]);
                a1[it] += (unsigned)(BK * sizeof(T));
            }
            glds16(rw2, &lds[buf][BM * KC + wbase], b1);
            b1 += (unsigned)(BK * sizeof(T));
        } else {
#pragma unroll
            for (int it = 0; it < A_IT; ++it) {
                glds16(rx, &lds[buf][wbase + it * NT], a2[it]);
                a2[it] += (unsigned)(BK * sizeof(T));
            }
            glds16(rw, &lds[buf][BM * KC + wbase], b2);
            b2 += (unsigned)(BK * sizeof(T));
        }
    };
    // the per-channel operands, 4 bytes per lane: even waves the 64 scales, odd waves the 64 shifts, of the main conv (the direct epilogue's aux
    // region) and of the inner one.  Issued BEFORE the first slab: older than everything a counted wait may leave in flight, so they have landed
    // at the first wait and are visible behind the first barrier.
    {
        const bool odd = __builtin_amdgcn_readfirstlane(wave) & 1;
        const int ch = n0 + lane;
        const float* src = odd ? p.shift : p.scale;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc_uniform(src, 0x7fffffffu);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(reinterpret_cast<unsigned*>(aux_lds) + (odd ? 64 : 0)), 4,
                                                 src ? (unsigned)ch * 4u : OOB, 0, 0, 0);
        const float* src2 = odd ? q.shift2 : q.scale2;
        const __amdgpu_buffer_rsrc_t rs2 = make_rsrc_uniform(src2, 0x7fffffffu);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs2, (__attribute__((address_space(3))) void*)(reinterpret_cast<unsigned*>(aux2_lds) + (odd ? 64 : 0)), 4,
                                                 src2 ? (unsigned)ch * 4u : OOB, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);

    f32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x4_t rres[TM][H];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int h = 0; h < H; ++h) rres[i][h] = u32x4_t{0u, 0u, 0u, 0u};

    const int fr = lane & 15, fq = lane >> 4;
    const unsigned aux2_addr = lds_addr(aux2_lds);
    const bool has_sc2 = q.scale2 != nullptr, has_sh2 = q.shift2 != nullptr;
    // the seam: acc = the inner conv, complete -> rres = bf16(acc * scale2 + shift2) in the residual registers' layout, acc = 0.  The same
    // multiply, add and single rounding as igemm_epilogue_direct / the staged epilogue perform for a launch without residual.
    auto seam = [&]() {
#pragma unroll
        for (int h = 0; h < H; ++h) {                           // (one 32-channel block at a time: 16 registers of scales / shifts, not 32)
            u32x4_t sc[2], sh[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned a = aux2_addr + (unsigned)(h * 32 + fq * 8 + k * 4) * 4u;
                sc[k] = frag_read<0>(a);
                sh[k] = frag_read<256>(a);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < 2; ++k) { asm volatile("" : "+v"(sc[k])); asm volatile("" : "+v"(sh[k])); }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] = acc[i][2 * h][e]; v[4 + e] = acc[i][2 * h + 1][e]; }
                if (has_sc2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] *= __uint_as_float(sc[0][e]); v[4 + e] *= __uint_as_float(sc[1][e]); }
                }
                if (has_sh2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] += __uint_as_float(sh[0][e]); v[4 + e] += __uint_as_float(sh[1][e]); }
                }
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) rres[i][h][qd] = pack2_bf16(v[2 * qd], v[2 * qd + 1]);
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    };

    // the three-level software pipeline of igemm_body's register-pipelined loop (its comments apply), over the S slabs of both convs
    constexpr int N_DMA = A_IT + 1;
    issue_slab(0, 0);
    if (S > 1) issue_slab(1, 1);
    if (S > 2) issue_slab(2, 2);
    __builtin_amdgcn_sched_barrier(0);
    constexpr unsigned SLAB_BYTES = SLOTS * 16;
    const int xrow = wm * (BM / WM) + fr, wrow = fr;
    const unsigned x_rd0 = lds_addr(&lds[0][0]) + (unsigned)(xrow * KC + swz<KC>(xrow, fq)) * 16u;
    const unsigned w_rd0 = lds_addr(&lds[0][0]) + (unsigned)((BM + wrow) * KC + swz<KC>(wrow, fq)) * 16u;
    u32x4_t xf0[TM], wf0[TN], xf1[TM], wf1[TN];
    if (S > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * N_DMA) : "memory");
    else if (S > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_DMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    frag_read_all<TM, KC * 16>(xf0, x_rd0);
    frag_read_all<TN, KC * 16>(wf0, w_rd0);
    frag_wait<TM, TN>(xf0, wf0);
    int rbuf = 1, ibuf = 0;
    auto step = [&](int s, u32x4_t* xc, u32x4_t* wc, u32x4_t* xn, u32x4_t* wn_) {
        const bool more = s + 1 < S;
        if (more) {
            if (s + 2 < S) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_DMA) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        // (unconditional reads and wait: see igemm_body)
        frag_read_all<TM, KC * 16>(xn, x_rd0 + (unsigned)rbuf * SLAB_BYTES);
        frag_read_all<TN, KC * 16>(wn_, w_rd0 + (unsigned)rbuf * SLAB_BYTES);
        if (more && s + 3 < S) issue_slab(s + 3, ibuf);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::run(wc[j], xc[i], acc[i][j]);
        frag_wait<TM, TN>(xn, wn_);
        rbuf = rbuf == NBUF - 1 ? 0 : rbuf + 1;
        ibuf = ibuf == NBUF - 1 ? 0 : ibuf + 1;
        if (s + 1 == S1) seam();                                // (block uniform; no asynchronous read is in flight here)
    };
    for (int s = 0; s < S; s += 2) {
        step(s, xf0, wf0, xf1, wf1);
        if (s + 1 < S) step(s + 1, xf1, wf1, xf0, wf0);
    }
    __builtin_amdgcn_sched_barrier(0);
    igemm_epilogue_direct<BM, BN, WM, WN, true, TWO>(p, acc, m0, n0, rres, lds_addr(aux_lds));
}

int launch_pair(const bool two, const ConvDev& d, const PairPre& q, hipStream_t st) {
    const dim3 grid(cdiv(d.M, 128), d.Cout / 64);
    if (two) hipLaunchKernelGGL((igemm_pair_kernel<true>), grid, dim3(256), 0, st, d, q);
    else hipLaunchKernelGGL((igemm_pair_kernel<false>), grid, dim3(256), 0, st, d, q);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
