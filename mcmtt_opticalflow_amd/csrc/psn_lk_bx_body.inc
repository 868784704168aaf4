// The body of the box-window LK kernel, included by each of its entries in
// psn_lk_bx.hip (lk_kernel_bx, lk_kernel_fw) inside the kernel's braces. In scope:
// the template parameters UPT, NOTAIL, NT, the launch arguments `A` (the kernel's
// own parameter) and the entry's policy type POL.
// Text, not a function template: read through an inlined function's parameter --
// by value or by reference -- the launch arguments stay a private copy of 4,352 B
// (the copy from the kernarg segment is not elided), every query field becomes
// a vector load from scratch, and the scalar J offsets no longer compile.
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    static_assert(UPT % 2 == 0, "units are processed in pairs");
    static_assert(NT == kBxNT || (NT == kBxNT2 && NOTAIL && UPT == kBxUPT2), "the two-wave build is <8, true>");
    constexpr int NW = NT / 64;             // waves
    constexpr bool QT = NT == kBxNT2;       // quarter-wave fallback tiles
    constexpr int TG = QT ? kBxTile2 : kBxTile;  // threads per fallback tile granule
    constexpr int TPH = 32 / TG;            // tiles per half wave (exactness is decided per half wave)
    // The chain lanes' tile step of the forward entry (POL::kChainNT; the two-wave
    // build measured no gain from it and keeps its loops): a full tile (all TG *
    // UPT units inside the window, one granule per tile) is NBF whole blocks per
    // lane chain in regions of stride SF
    // in planes of pitch PF wherever it lies in the window, so the chain lanes take
    // their region offset once per fallback and sum the tile by chain_sum_nt<NBF>.
    // A partial last tile keeps bx_tile_slots_nt and chain_sum_pl.
    constexpr bool CNT = NOTAIL && POL::kChainNT;
    constexpr int NBF = bx_nt_tile_blocks(UPT, TG), SF = bx_nt_tile_S(UPT, TG), PF = bx_nt_tile_P(UPT, TG);
    static_assert(!CNT || NBF * 16 == TG * UPT, "a full no-tail tile is whole blocks");
    const int tid = threadIdx.x, lane = tid & 63;
    if (A.poison_lds) lds_poison<NT>(smem, A.poison_lds);
    const int g = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    int qi = 0;
    while (qi + 1 < A.nq && g >= A.q[qi + 1].wg_begin) qi++;
    const LkQueryDev &Q = A.q[qi];
    const int pi = lk_query_point(Q, A.counts, A.count_stride, g);
    if (pi < 0) return;  // past the query's device count
    const int w = Q.win_w, h = Q.win_h;
    const int maxL = Q.max_level, flags = Q.flags;
    const bool sse = (flags & PSN_LK_ACCUM_SCALAR) == 0;
    const int QW = bx_qw(w), U = h * QW;
    const int nqB = sse ? (w / 8) * 2 : 0, n8 = 4 * nqB, tB = w - n8;   // b: 8-pixel steps
    const int nqA = sse ? w / 4 : 0, nA4 = 4 * nqA, tA = w - nA4;        // A: 4-pixel steps
    const int PM = bx_pm(w), JRW = st_jreg_w(w), JRH = st_jreg_h(h), JRP = bx_jrp(w), JRP4 = JRP >> 2;
    const BxLayout lay(w, h, UPT, 1, TG);
    int *X = (int *)smem;                      // chain-check records, two parities
    float *RS = (float *)(X + kBxXInts);       // serial-chain results (wave 0 -> all)
    int *EP = (int *)(RS + 16);                // err partial sums per wave
    // b-fallback tile hand-off flags (the split path below): ready[3], consumed[3], and
    // FLG[6] = a hand-off wait ran out of its bound (never expected: the point is
    // then reported failed, see the result writes)
    volatile int *FLG = (volatile int *)(RS + 24);
    if (threadIdx.x < 7) FLG[threadIdx.x] = threadIdx.x < 6 ? -1 : 0;  // ordered by the first level barrier
    if constexpr (NW < 4) {
        // the records of the absent waves, once per parity (no wave ever writes
        // them): totals 0, verdict "none" -- bx_check / bx_eval read four waves
        if (tid < kBxRecInts) {
            const int v = tid < kBxHalfRec ? 0 : 8;
            if ((tid & 3) >= NW) X[tid] = X[4 * kBxRecInts + tid] = v;
        }
    }
    int fb_epoch = 0;
    uint8_t *JR = smem + lay.jr;
    const uint32_t *JR32 = (const uint32_t *)JR;
    uint8_t *UN = smem + lay.un;
    const uint32_t *P32 = (const uint32_t *)UN;
    float *PL = (float *)UN;

    const int u0 = tid * UPT;
    const int y0 = u0 / QW, q0 = u0 - y0 * QW;
    // per unit of the thread: the byte offset of its J dwords in the region (row
    // y * JRP + 4 q; 0 past the window, where the gradients are zero), two units
    // per register (the b pass adds a half to the iteration's base: SDWA), and
    // whether it is an SSE2 unit of the b chains (bit k)
    unsigned UB[UPT / 2];
    unsigned sseB = 0;
    {
        int y = y0, q = q0;
#pragma unroll
        for (int k = 0; k < UPT; k++) {
            const unsigned o = u0 + k < U ? (unsigned)(y * JRP + 4 * q) : 0u;
            if (k & 1)
                UB[k >> 1] |= o << 16;
            else
                UB[k >> 1] = o;
            sseB |= (unsigned)(q < nqB) << k;
            if (++q == QW) {
                q = 0;
                y++;
            }
        }
    }

    const float hwx = __fmul_rn((float)(w - 1), 0.5f), hwy = __fmul_rn((float)(h - 1), 0.5f);
    const float px0 = A.prev[2 * pi], py0 = A.prev[2 * pi + 1];
    float NPx = 0.f, NPy = 0.f;
    if (flags & PSN_LK_USE_INITIAL_FLOW) {
        NPx = A.next[2 * pi];
        NPy = A.next[2 * pi + 1];
    }
    int status = 1;
    float errv = 0.f;
    int par = 0;
#ifdef PSN_LK_STAMPS
    unsigned long long bx_acc[16] = {}, bx_t = 0, bx_t0 = 0, bx_r0 = 0, bx_te = 0;
    // the fallback tile splits (stamps 19-30) add up in the 16 free words of the
    // scratch region, by thread 0 alone: as registers they spill in every build
    unsigned *bx_tl = (unsigned *)(RS + 32);
    if (threadIdx.x < 14) bx_tl[threadIdx.x] = 0;  // ordered by the first level barrier
#define BX_TL(slot, d)                                      \
    do {                                                    \
        if (threadIdx.x == 0) bx_tl[(slot)-19] += (unsigned)(d); \
    } while (0)
    PSN_CLK_ORDERED(bx_t0);
    bx_t = bx_t0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(bx_r0) : : "memory");  // 100 MHz
#endif

    unsigned IP[UPT][2], XP[UPT][2], YP[UPT][2];  // I, Ix, Iy as packed 16-bit pairs (pixels 0,1 and 2,3)
    int gmax = 0;              // max |Ix|, |Iy| of the thread's pixels
    unsigned nwin = 0;         // window passes (A phase + iterations) over the levels: the sample count / (w*h)

    for (int level = maxL; level >= 0; level--) {
        const LevelDev I = ring_level_u(A.ring, Q.prev_slot, level);
        const LevelDev J = ring_level_u(A.ring, Q.next_slot, level);
        const int cols = I.w, rows = I.h;
        const float scale = ldexpf(1.f, -level);
        float px = __fmul_rn(px0, scale), py = __fmul_rn(py0, scale);
        float nx, ny;
        if (level == maxL) {
            if (flags & PSN_LK_USE_INITIAL_FLOW) {
                nx = __fmul_rn(NPx, scale);
                ny = __fmul_rn(NPy, scale);
            } else {
                nx = px;
                ny = py;
            }
        } else {
            nx = __fmul_rn(NPx, 2.f);
            ny = __fmul_rn(NPy, 2.f);
        }
        NPx = nx;
        NPy = ny;
        px = __fsub_rn(px, hwx);
        py = __fsub_rn(py, hwy);
        const int ipx = cv_floor(px), ipy = cv_floor(py);
        if (win_outside(ipx, ipy, w, h, cols, rows)) {
            if (level == 0) {
                status = 0;
                errv = 0.f;
            }
            continue;
        }
        int iw00, iw01, iw10, iw11;
        bilin_weights(__fsub_rn(px, (float)ipx), __fsub_rn(py, (float)ipy), iw00, iw01, iw10, iw11);
        nx = __fsub_rn(nx, hwx);
        ny = __fsub_rn(ny, hwy);
        int jr_x0 = (cv_floor(nx) - kStJMargin) & ~3, jr_y0 = cv_floor(ny) - kStJMargin;

        __syncthreads();  // the previous level is done with LDS
        dma_patch<NT>(UN, I, ipy - 1, ipx - 1, w + 3, h + 3, PM, Q.dv_bxpm);
        dma_wait();
        // the J region moves while the A phase reads the I patch: waited for
        // before the A publish barrier, which makes it visible to every wave
        dma_patch<NT>(JR, J, jr_y0, jr_x0, JRW, JRH, JRP4, Q.dv_bxjr);
        barrier_inflight();  // the I patch (waited above) for every wave; J still moving
        PSN_PH_MARK(bx_acc, bx_t, 0);  // level setup + staging
        bx_prio_lo();

        // ---- A phase: Scharr + bilinear window values of the thread's units from
        // the I patch bytes; the 15 A chains (sum x class) as runs ----
        float sA[3];  // the raw A11, A12, A22 sums
        nwin++;
        // the two-wave build alone has the sliding A pass (uniform per query: a scalar branch)
        const bool slide = QT && bx_slides(w, NT);
        {
            const int sh = (ipx - 1) & 3;
            int T11[5] = {0, 0, 0, 0, 0}, T22[5] = {0, 0, 0, 0, 0}, T12[5] = {0, 0, 0, 0, 0};
            int M12[5] = {0, 0, 0, 0, 0}, m12[5] = {0, 0, 0, 0, 0};
            int gmx = 0, gmn = 0;  // max / min gradient of the thread's pixels
            // every derivative the window reads inside the image (columns ipx .. ipx +
            // 4 QW + 1, rows ipy .. ipy + h): no border masks (uniform)
            const bool interior = ipx >= 0 && ipy >= 0 && ipx + 4 * QW + 2 <= cols && ipy + h + 1 <= rows;
            const int c256 = 1 << 8, c8192 = 1 << 13;  // scalar accumulators of the VOP3 v_dot2
            auto apass = [&](auto inner, auto slideT) {
            constexpr bool IN = decltype(inner)::value;
            int y = y0, q = q0;
            asm volatile("" : "+v"(y), "+v"(q));  // opaque: no per-unit address hoisting (VGPRs)
            if constexpr (decltype(slideT)::value) {
                // the sliding pass (bx_slides: the run is UPT adjacent quads of one window
                // row, all inside the window or all past it): the first unit in full, each
                // later one from its left neighbour's carry and one new dword per row.
                // A run past the window reads the quads of row 0 with zero weights: zero
                // gradients (and I values nothing reads: the thread's gmax is 0, and the
                // fallback writers and the err pass skip units past U)
                const bool uv = u0 < U;
                const int yy = uv ? y : 0, qq = uv ? q : 0;
                const uint32_t *p0 = P32 + yy * PM + qq;
                const unsigned Wa = uv ? pack_w(iw00, iw01) : 0u, Wb = uv ? pack_w(iw10, iw11) : 0u;
                BxCarry C;
#pragma unroll
                for (int k = 0; k < UPT; k++) {
                    if (k == 0)
                        bx_unit_slide<IN, true>(p0, PM, sh, yy, qq, ipx, ipy, cols, rows, Wa, Wb, c256, c8192, C, IP[k],
                                                XP[k], YP[k], gmx, gmn);
                    else
                        bx_unit_slide<IN, false>(p0 + k, PM, sh, yy, qq + k, ipx, ipy, cols, rows, Wa, Wb, c256, c8192, C,
                                                 IP[k], XP[k], YP[k], gmx, gmn);
                    // materialize the unit's results and its carry here (as below)
                    asm volatile("" : "+v"(IP[k][0]), "+v"(IP[k][1]), "+v"(XP[k][0]), "+v"(XP[k][1]), "+v"(YP[k][0]),
                                 "+v"(YP[k][1]), "+v"(gmx), "+v"(gmn));
                    if (k + 1 < UPT) {
                        asm volatile("" : "+v"(C.d2[0]), "+v"(C.d2[1]), "+v"(C.d2[2]), "+v"(C.d2[3]), "+v"(C.E[0][0]),
                                     "+v"(C.E[0][1]), "+v"(C.E[1][0]), "+v"(C.E[1][1]), "+v"(C.DX[0]), "+v"(C.DX[1]),
                                     "+v"(C.DY[0]), "+v"(C.DY[1]));
                        asm volatile("" : "+v"(C.SV[0][0]), "+v"(C.SV[0][1]), "+v"(C.SV[1][0]), "+v"(C.SV[1][1]),
                                     "+v"(C.DV[0][0]), "+v"(C.DV[0][1]), "+v"(C.DV[1][0]), "+v"(C.DV[1][1]));
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one unit at a time (register pressure)
                }
                return;
            }
#pragma unroll
            for (int k = 0; k < UPT; k++) {
                const bool uv = u0 + k < U;
                const int yy = uv ? y : 0, qq = uv ? q : 0;
                bx_unit<IN, NOTAIL>(P32, PM, sh, yy, qq, uv, w, ipx, ipy, cols, rows, iw00, iw01, iw10, iw11, c256,
                                    c8192, IP[k], XP[k], YP[k], gmx, gmn);
                // materialize the unit's results here: no sinking of its arithmetic
                // past later units (which would keep its patch bytes live)
                asm volatile("" : "+v"(IP[k][0]), "+v"(IP[k][1]), "+v"(XP[k][0]), "+v"(XP[k][1]), "+v"(YP[k][0]),
                             "+v"(YP[k][1]), "+v"(gmx), "+v"(gmn));
                if (++q == QW) {
                    q = 0;
                    y++;
                }
                __builtin_amdgcn_sched_barrier(0);  // one unit at a time (register pressure)
            }
            };
            if constexpr (QT) {
                if (slide && interior)
                    apass(std::true_type(), std::true_type());
                else if (slide)
                    apass(std::false_type(), std::true_type());
            }
            if (!slide && interior)
                apass(std::true_type(), std::false_type());
            else if (!slide)
                apass(std::false_type(), std::false_type());
            gmax = max(gmx, -gmn);
            // A products of the window values, units in pairs (a second pass keeps
            // the Scharr temporaries and the chain runs apart): v_mad_i32_i16 on the
            // packed gradient halves, one v_max3 / v_min3 per two A12 prefixes
            int q = q0;
            asm volatile("" : "+v"(q));
#pragma unroll
            for (int k = 0; k < UPT; k += 2) {
                unsigned xs[2][2], ys[2][2], xt[2][2], yt[2][2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    // SSE2 unit: pixel i feeds lane chain i; else the tail chain, row-major
                    // (branch-free: the other chain's gradients are masked to zero)
                    const unsigned ms = (NOTAIL || q < nqA) ? ~0u : 0u;
#pragma unroll
                    for (int hh = 0; hh < 2; hh++) {
                        xs[u][hh] = XP[k + u][hh] & ms;
                        ys[u][hh] = YP[k + u][hh] & ms;
                        xt[u][hh] = XP[k + u][hh] & ~ms;
                        yt[u][hh] = YP[k + u][hh] & ~ms;
                    }
                    if (++q == QW) q = 0;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int hh = i >> 1;
                    int ta, tb;
                    if (i & 1) {
                        T11[i] = mad16p<1, 1>(xs[1][hh], xs[1][hh], mad16p<1, 1>(xs[0][hh], xs[0][hh], T11[i]));
                        T22[i] = mad16p<1, 1>(ys[1][hh], ys[1][hh], mad16p<1, 1>(ys[0][hh], ys[0][hh], T22[i]));
                        ta = mad16p<1, 1>(xs[0][hh], ys[0][hh], T12[i]);
                        tb = mad16p<1, 1>(xs[1][hh], ys[1][hh], ta);
                    } else {
                        T11[i] = mad16p<0, 0>(xs[1][hh], xs[1][hh], mad16p<0, 0>(xs[0][hh], xs[0][hh], T11[i]));
                        T22[i] = mad16p<0, 0>(ys[1][hh], ys[1][hh], mad16p<0, 0>(ys[0][hh], ys[0][hh], T22[i]));
                        ta = mad16p<0, 0>(xs[0][hh], ys[0][hh], T12[i]);
                        tb = mad16p<0, 0>(xs[1][hh], ys[1][hh], ta);
                    }
                    run2(T12[i], M12[i], m12[i], ta, tb);
                }
                if (!NOTAIL) {  // the tail chain: unit k's pixels 0-3, then unit k+1's
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int hh = 0; hh < 2; hh++) {
                            T11[4] = mad16p<1, 1>(xt[u][hh], xt[u][hh], mad16p<0, 0>(xt[u][hh], xt[u][hh], T11[4]));
                            T22[4] = mad16p<1, 1>(yt[u][hh], yt[u][hh], mad16p<0, 0>(yt[u][hh], yt[u][hh], T22[4]));
                            const int ta = mad16p<0, 0>(xt[u][hh], yt[u][hh], T12[4]);
                            const int tb = mad16p<1, 1>(xt[u][hh], yt[u][hh], ta);
                            run2(T12[4], M12[4], m12[4], ta, tb);
                        }
                }
                asm volatile("" : "+v"(T11[0]), "+v"(T11[1]), "+v"(T11[2]), "+v"(T11[3]), "+v"(T11[4]), "+v"(T22[0]),
                             "+v"(T22[1]), "+v"(T22[2]), "+v"(T22[3]), "+v"(T22[4]));
                asm volatile("" : "+v"(T12[0]), "+v"(T12[1]), "+v"(T12[2]), "+v"(T12[3]), "+v"(T12[4]), "+v"(M12[0]),
                             "+v"(M12[1]), "+v"(M12[2]), "+v"(M12[3]), "+v"(M12[4]));
                asm volatile("" : "+v"(m12[0]), "+v"(m12[1]), "+v"(m12[2]), "+v"(m12[3]), "+v"(m12[4]));
            }
            // A11 / A22 terms are >= 0: the maximum prefix is the total
            int T[15], M[15], m[15];
#pragma unroll
            for (int c = 0; c < 5; c++) {
                T[c] = T11[c], M[c] = T11[c], m[c] = 0;
                T[5 + c] = T12[c], M[5 + c] = M12[c], m[5 + c] = m12[c];
                T[10 + c] = T22[c], M[10 + c] = T22[c], m[10 + c] = 0;
            }
            PSN_PH_MARK(bx_acc, bx_t, 1);  // A window values + runs
            bx_prio_hi();
            int *rec = X + par * 4 * kBxRecInts;
            par ^= 1;
            bx_publish<15>(T, rec, NOTAIL || tA == 0);
            dma_wait();  // this thread's J region loads (the barrier: every thread's)
            __syncthreads();
            bx_check<15>(T, M, m, false, rec, NOTAIL || tA == 0);
            __syncthreads();
            int tot, h0, base0;
            const bool exact = bx_eval<15>(rec, tot, h0, base0);
            if (exact) {
#pragma unroll
                for (int s = 0; s < 3; s++) sA[s] = combine_a5([&](int i) { return rl_f(tot, i); }, s, sse);
            } else {
                // ordered float chains from half wave h0 on (every earlier prefix is an
                // exact integer: the chains start from base0): tiles of HW half waves
                // (the units of threads 32g..), products chain-major into 3 planes,
                // double-buffered: the threads of the next tile write its products
                // while the chain lanes (lanes 0-14 of wave 0; lane c holds chain c's
                // base0) sum the current one
                // the fallback's thread roles from an opaque copy of the thread id: computed
                // here, not hoisted to the kernel start and spilled across the loops
                int ftid = (int)threadIdx.x;
                asm volatile("" : "+v"(ftid));
                const int HW = QT ? 1 : Q.bx_hw, PCA = 3 * bx_pc(UPT, TG) * HW;
                const bool chl = ftid < 15;  // wave 0: its tiles are written first, so it rarely writes while it sums
                const int cl = chl ? ftid : 0, cs = cl / 5, cc = cl - 5 * cs;
                float acc = (float)base0;  // |base0| <= 2^24: exact
                const int g_last = (U - 1) / (TG * UPT), g_first = h0 * TPH;
                // The tile's chain slots (bx_tile_slots). No-tail builds take the short form
                // (bx_tile_slots_nt: no division on the tile loop's path) everywhere but in the
                // half-wave writers, writeA_nt and the b fallback's write_tile_nt (shortT
                // false): those hold the register peak of the <4 / 8 / 10, true> builds,
                // which moves with the form (121 / 151 / 164 for 122 / 152 / 167, the
                // figures tests/test_bx_two_wave_plan.py holds them to). The forward
                // entry (POL::kShortWriterGeo) takes the short form there as well.
                auto geoA_g = [&](int g, int &sa, int &ta, int &nsse, int &ntail, auto shortT) {
                    const int ua = TG * UPT * g, ub = min(ua + TG * UPT * HW, U);
                    if constexpr (NOTAIL && (decltype(shortT)::value || POL::kShortWriterGeo)) {
                        static_assert((TG * UPT) % 16 == 0, "a full no-tail tile has no pad");
                        bx_tile_slots_nt(ua, ub, sa, ta, nsse, ntail);
                    } else {
                        bx_tile_slots(ua, ub, QW, nqA, nA4, tA, sa, ta, nsse, ntail);
                    }
                };
                auto geoA = [&](int g, int &sa, int &ta, int &nsse, int &ntail) {
                    geoA_g(g, sa, ta, nsse, ntail, std::true_type());
                };
                auto unitA = [&](int yk, int qk, bool uv, unsigned x0, unsigned x1, unsigned y0_, unsigned y1_, float *buf,
                                 int S, int P, int sa, int ta) {
                    if (!uv) return;
                    unsigned xp[2] = {x0, x1}, yp[2] = {y0_, y1_};
                    asm volatile("" : "+v"(xp[0]), "+v"(xp[1]), "+v"(yp[0]), "+v"(yp[1]));
                    const bool su = NOTAIL || qk < nqA;
                    const int base = su ? yk * nqA + qk - sa : 4 * S + yk * tA + 4 * qk - nA4 - ta;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        // pixels past the window width write a dummy slot past the buffers
                        const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                        const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                        const bool on = 4 * qk + i < w;
                        float *d1 = on ? buf + (su ? i * S + base : base + i) : PL + 2 * PCA;
                        const int pp = on ? P : 1;
                        d1[0] = (float)__mul24(gx, gx);
                        d1[pp] = (float)__mul24(gx, gy);
                        d1[2 * pp] = (float)__mul24(gy, gy);
                    }
                };
                // half-wave tiles: the whole wave writes one (as the b fallback's write_tile)
                constexpr int K1 = UPT / 2;
                const bool split = !QT && HW == 1 && (UPT & 1) == 0;
                auto swp = [](unsigned a, unsigned b, bool first) {
                    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                    return first ? r[0] : r[1];
                };
                // no-tail build: the tile's half picked at compile time, the unit's plane
                // slot from its index in the tile (as the b fallback's write_tile_nt)
                auto writeA_nt = [&](int g, float *buf, auto lowerT) {
                    constexpr bool lower = decltype(lowerT)::value;
                    if ((ftid >> 6) != (g >> 1)) return;
                    int sa, ta, nsse, ntail;
                    geoA_g(g, sa, ta, nsse, ntail, std::false_type());  // (the general form: see geoA_g)
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const bool up = (ftid & 32) != 0;
                    const int ub = lower ? (up ? (ftid ^ 32) * UPT + K1 : ftid * UPT) : (up ? ftid * UPT + K1 : (ftid ^ 32) * UPT);
                    const int rel = ub - 32 * UPT * g;
                    auto pick = [](unsigned a, unsigned b) {
                        auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                        return lower ? r[0] : r[1];
                    };
#pragma unroll
                    for (int k = 0; k < K1; k++) {
                        unsigned xp[2] = {pick(XP[k][0], XP[K1 + k][0]), pick(XP[k][1], XP[K1 + k][1])};
                        unsigned yp[2] = {pick(YP[k][0], YP[K1 + k][0]), pick(YP[k][1], YP[K1 + k][1])};
                        if (ub + k < U) {
                            asm volatile("" : "+v"(xp[0]), "+v"(xp[1]), "+v"(yp[0]), "+v"(yp[1]));
                            // (bx_store_a written out: through the helper <16, true> runs 0.7 % slower)
                            float *d1 = buf + rel + k;
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                                const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                                d1[i * S] = (float)__mul24(gx, gx);
                                d1[i * S + P] = (float)__mul24(gx, gy);
                                d1[i * S + 2 * P] = (float)__mul24(gy, gy);
                            }
                        }
                    }
                };
                // two-wave build, quarter-wave tiles: the tile's wave writes it with all
                // four rows -- row r takes the units 2r, 2r + 1 of the tile's threads
                // (bx_qpick over the unit pairs' registers), the quarter picked at
                // compile time; slots from the unit's index in the tile
                auto writeA_q = [&](int g, float *buf, auto tqT) __attribute__((always_inline)) {
                    constexpr int TQ = decltype(tqT)::value;
                    int sa, ta, nsse, ntail;
                    geoA(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const int rel = (ftid & 15) * UPT + 2 * ((ftid >> 4) & 3), ub = TG * UPT * g + rel;
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        unsigned xp[2] = {bx_qpick<TQ>(XP[j][0], XP[2 + j][0], XP[4 + j][0], XP[6 + j][0]),
                                          bx_qpick<TQ>(XP[j][1], XP[2 + j][1], XP[4 + j][1], XP[6 + j][1])};
                        unsigned yp[2] = {bx_qpick<TQ>(YP[j][0], YP[2 + j][0], YP[4 + j][0], YP[6 + j][0]),
                                          bx_qpick<TQ>(YP[j][1], YP[2 + j][1], YP[4 + j][1], YP[6 + j][1])};
                        if (ub + j < U) {
                            asm volatile("" : "+v"(xp[0]), "+v"(xp[1]), "+v"(yp[0]), "+v"(yp[1]));
                            // (bx_store_a written out: through the helper this build runs 0.5 % slower)
                            float *d1 = buf + rel + j;
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                                const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                                d1[i * S] = (float)__mul24(gx, gx);
                                d1[i * S + P] = (float)__mul24(gx, gy);
                                d1[i * S + 2 * P] = (float)__mul24(gy, gy);
                            }
                        }
                    }
                };
                auto writeA = [&](int g, float *buf) {
                    if constexpr (NOTAIL) {
                        if (HW == 1) {  // (split: UPT is even)
                            if (g & 1)
                                writeA_nt(g, buf, std::false_type());
                            else
                                writeA_nt(g, buf, std::true_type());
                            return;
                        }
                    }
                    int sa, ta, nsse, ntail;
                    if (split) {
                        if ((ftid >> 6) != (g >> 1)) return;
                        geoA(g, sa, ta, nsse, ntail);
                        const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                        const bool lower = (g & 1) == 0, own = ((ftid >> 5) & 1) == (g & 1);
                        const int ub = (own ? ftid : ftid ^ 32) * UPT + (lower == own ? 0 : K1);
                        int yk = ub / QW, qk = ub - yk * QW;
                        asm volatile("" : "+v"(yk), "+v"(qk));
#pragma unroll
                        for (int k = 0; k < K1; k++) {
                            unitA(yk, qk, ub + k < U, swp(XP[k][0], XP[K1 + k][0], lower), swp(XP[k][1], XP[K1 + k][1], lower),
                                  swp(YP[k][0], YP[K1 + k][0], lower), swp(YP[k][1], YP[K1 + k][1], lower), buf, S, P, sa, ta);
                            if (++qk == QW) {
                                qk = 0;
                                yk++;
                            }
                        }
                        return;
                    }
                    if ((ftid >> 5) < g || (ftid >> 5) >= g + HW) return;
                    geoA(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    if constexpr (NOTAIL && UPT <= 8) {  // the thread's own units, slots from their index
                        const int rel = u0 - 32 * UPT * g;
#pragma unroll
                        for (int k = 0; k < UPT; k++) {
                            if (u0 + k >= U) break;
                            unsigned xp[2] = {XP[k][0], XP[k][1]}, yp[2] = {YP[k][0], YP[k][1]};
                            asm volatile("" : "+v"(xp[0]), "+v"(xp[1]), "+v"(yp[0]), "+v"(yp[1]));
                            bx_store_a(buf + rel + k, xp, yp, S, P);
                        }
                        return;
                    }
                    int yk = y0, qk = q0;
                    asm volatile("" : "+v"(yk), "+v"(qk));
#pragma unroll
                    for (int k = 0; k < UPT; k++) {
                        unitA(yk, qk, u0 + k < U, XP[k][0], XP[k][1], YP[k][0], YP[k][1], buf, S, P, sa, ta);
                        if (++qk == QW) {
                            qk = 0;
                            yk++;
                        }
                    }
                };
                // the tile writer of the build. (The two-wave build's is always inlined, and
                // generic so that only that build instantiates it: as a call its four
                // quarter bodies would keep the by-reference captures in scratch.)
                auto writeA_qt = [&](int g, float *buf, auto) __attribute__((always_inline)) {
                    if ((ftid >> 6) != (g >> 2)) return;
                    switch (g & 3) {
                        case 0: writeA_q(g, buf, std::integral_constant<int, 0>()); break;
                        case 1: writeA_q(g, buf, std::integral_constant<int, 1>()); break;
                        case 2: writeA_q(g, buf, std::integral_constant<int, 2>()); break;
                        default: writeA_q(g, buf, std::integral_constant<int, 3>()); break;
                    }
                };
                auto padA = [&](int g, float *buf) {  // chain lanes: zero their region's pad
                    if (!chl) return;
                    int sa, ta, nsse, ntail;
                    geoA(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const int len = cc < 4 ? nsse : ntail;
                    float *rg = buf + cs * P + cc * S;
                    for (int i = len; i < ((len + 15) & ~15); i++) rg[i] = 0.f;
                };
                // the I patch under PL was consumed before the publish barrier
                if constexpr (QT)
                    writeA_qt(g_first, PL, 0);
                else
                    writeA(g_first, PL);
                padA(g_first, PL);
                __syncthreads();
                // (CNT) once per fallback: the chain lane's region offset in a full tile
                [[maybe_unused]] const int roff = cs * PF + cc * SF;
                [[maybe_unused]] const bool one = HW == 1;  // one granule per tile: a tile inside the window is full
                for (int g = g_first, t = 0; g <= g_last; g += HW, t ^= 1) {
                    float *cur = PL + t * PCA, *nxt = PL + (t ^ 1) * PCA;
#ifdef PSN_LK_STAMPS
                    unsigned long long tc0, tc1, tc2, tc3, tc4, tc5;
                    PSN_CLK_ORDERED(tc0);
#endif
                    if (g + HW <= g_last) {
                        if constexpr (QT)
                            writeA_qt(g + HW, nxt, 0);
                        else
                            writeA(g + HW, nxt);
                    }
#ifdef PSN_LK_STAMPS
                    PSN_CLK_ORDERED(tc1);
                    tc2 = tc3 = tc1;
#endif
                    bool full = false;  // (CNT) the straight-line step of a full tile
                    if constexpr (CNT) full = one && TG * UPT * (g + 1) <= U;
                    if constexpr (CNT) {
                        if (full && (ftid >> 6) == 0) {
                            PSN_CLK_ORDERED(tc2);
                            if (chl && cc < 4) acc = chain_sum_nt<NBF>(cur + roff, acc PSN_STAMPS_ONLY(, &bx_tl[24 - 19]));
                            PSN_CLK_ORDERED(tc3);
                            // only the window's last tile can have a pad
                            if (g + 1 == g_last) padA(g_last, nxt);
                        }
                    }
                    if (!full && (ftid >> 6) == 0) {
                        int sa, ta, nsse, ntail;
                        geoA(g, sa, ta, nsse, ntail);
                        const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                        const int len = chl ? (cc < 4 ? nsse : ntail) : 0;
                        // (no-tail: every chain lane's length is nsse)
                        const int nbmax = NOTAIL ? (nsse + 15) >> 4 : __builtin_amdgcn_readlane(wave_max_scan((len + 15) >> 4), 63);
                        PSN_CLK_ORDERED(tc2);
                        // (no-tail: the tail-chain lanes keep acc = 0)
                        if (chl && (!NOTAIL || cc < 4))
                            acc = chain_sum_pl<NOTAIL>(cur + cs * P + cc * S, len, nbmax, acc PSN_STAMPS_ONLY(, &bx_tl[24 - 19]));
                        PSN_CLK_ORDERED(tc3);
                        if (g + HW <= g_last) padA(g + HW, nxt);
                    }
#ifdef PSN_LK_STAMPS
                    PSN_CLK_ORDERED(tc4);
#endif
                    __syncthreads();
#ifdef PSN_LK_STAMPS
                    PSN_CLK_ORDERED(tc5);  // (chain lane 0's view, as the b fallback's stamps below)
                    BX_TL(19, tc1 - tc0);                  // its wave's write of the next tile
                    BX_TL(20, (tc2 - tc1) + (tc4 - tc3));  // geometry + pad
                    BX_TL(21, tc3 - tc2);                  // chain sums (first-block wait: 24)
                    BX_TL(22, tc5 - tc4);                  // barrier wait
                    BX_TL(23, 1);
#endif
                }
                if (ftid < 64) {  // wave 0 combines in the SSE2 build's order
#pragma unroll
                    for (int s = 0; s < 3; s++) {
                        const float t = combine_a5([&](int i) { return readlane_f(acc, i); }, s, sse);
                        if (ftid == 0) RS[s] = t;
                    }
                }
                __syncthreads();
                sA[0] = RS[0];
                sA[1] = RS[1];
                sA[2] = RS[2];
            }
            PSN_PH_MARK(bx_acc, bx_t, 2);  // A publish / eval / serial chains
        }
        const LkSolve S = lk_solve(sA[0], sA[1], sA[2], w * h, Q.min_eig);
        if (flags & PSN_LK_GET_MIN_EIGENVALS) errv = S.minEig;
        if (!S.ok) {
            if (level == 0) status = 0;
            continue;
        }

        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < Q.max_count; j++) {
            const int inx = cv_floor(nx), iny = cv_floor(ny);
            if (win_outside(inx, iny, w, h, cols, rows)) {
                if (level == 0) status = 0;
                break;
            }
            int w00, w01, w10, w11;
            bilin_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny), w00, w01, w10, w11);
            if (!(jr_covers(inx, iny, w, h, jr_x0, jr_y0, JRW, JRH))) {
                // every wave's J reads of the previous iteration precede its barrier
                jr_x0 = (inx - kStJMargin) & ~3;
                jr_y0 = iny - kStJMargin;
                dma_patch<NT>(JR, J, jr_y0, jr_x0, JRW, JRH, JRP4, Q.dv_bxjr);
                dma_wait();
                __syncthreads();
            }
            PSN_PH_MARK(bx_acc, bx_t, 3);  // iteration head (restage)
            bx_prio_lo();
            PSN_PH_COUNT(bx_acc, 10);
            nwin++;
            const unsigned W0 = pack_w(w00, w01), W1 = pack_w(w10, w11);
            const int ox = inx - jr_x0, oy = iny - jr_y0, sj = ox & 3;
            const unsigned s0 = bx_sel(sj, 0), s1 = bx_sel(sj, 1), s2 = bx_sel(sj, 2), s3 = bx_sel(sj, 3);
            int T1[5] = {0, 0, 0, 0, 0}, M1[5] = {0, 0, 0, 0, 0}, m1[5] = {0, 0, 0, 0, 0};
            int T2[5] = {0, 0, 0, 0, 0}, M2[5] = {0, 0, 0, 0, 0}, m2[5] = {0, 0, 0, 0, 0};
            int dmx = 0, dmn = 0;  // max / min d of the thread's pixels (when tracked)
            const int c256 = opaque256();
            // every term d * g is an exact float unless |g| > 2^24 / 8160 (|d| <= 8160):
            // below that in the whole wave, the pass keeps no max |d|
            const bool dtrack = __ballot(gmax > kExact / 8160) != 0ull;
            auto bmain = [&](auto trk) {
                // the iteration's byte offsets of rows oy and oy + 1 in LDS, opaque
                // scalars (the J region's constant offset stays inside them: one
                // SDWA add per row and unit, not two adds and a constant)
                unsigned jo0 = (unsigned)((const uint8_t *)(JR32 + oy * JRP4 + (ox >> 2)) - smem);
                // (the two-wave build: the compiler does not prove the offset uniform; it is)
                if constexpr (QT) jo0 = (unsigned)__builtin_amdgcn_readfirstlane((int)jo0);
                unsigned jo1 = jo0 + 4u * (unsigned)JRP4;
                asm volatile("" : "+s"(jo0), "+s"(jo1));
                // units in pairs (UPT is even): each chain takes its two terms by
                // v_mad_i32_i16 (gradient half, product and sum in one) and one
                // v_max3 / v_min3 of the two new prefixes
#pragma unroll
                for (int k = 0; k < UPT; k += 2) {
                    int d[2][4], ms[2];
                    asm volatile("" : "+v"(UB[k >> 1]));  // opaque per iteration: its halves stay packed
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const unsigned o = u ? UB[k >> 1] >> 16 : UB[k >> 1] & 0xffffu;
                        bx_diffs2((const uint32_t *)(smem + jo0 + o), (const uint32_t *)(smem + jo1 + o), W0, W1, s0, s1, s2,
                                  s3, IP[k + u], d[u], c256);
                        ms[u] = -(int)((sseB >> (k + u)) & 1u);  // SSE2 unit -> lane chains 0-3, else the tail chain
                    }
                    if constexpr (decltype(trk)::value) {
#pragma unroll
                        for (int u = 0; u < 2; u++) {
                            dmx = max(dmx, max(d[u][0], d[u][1]));
                            dmx = max(dmx, max(d[u][2], d[u][3]));
                            dmn = min(dmn, min(d[u][0], d[u][1]));
                            dmn = min(dmn, min(d[u][2], d[u][3]));
                        }
                    }
                    if (NOTAIL) {  // every unit feeds lane chains 0-3
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int h = i >> 1;
                            int ta, tb;
                            if (i & 1) {
                                ta = mad16<1>(d[0][i], XP[k][h], T1[i]);
                                tb = mad16<1>(d[1][i], XP[k + 1][h], ta);
                            } else {
                                ta = mad16<0>(d[0][i], XP[k][h], T1[i]);
                                tb = mad16<0>(d[1][i], XP[k + 1][h], ta);
                            }
                            run2(T1[i], M1[i], m1[i], ta, tb);
                            if (i & 1) {
                                ta = mad16<1>(d[0][i], YP[k][h], T2[i]);
                                tb = mad16<1>(d[1][i], YP[k + 1][h], ta);
                            } else {
                                ta = mad16<0>(d[0][i], YP[k][h], T2[i]);
                                tb = mad16<0>(d[1][i], YP[k + 1][h], ta);
                            }
                            run2(T2[i], M2[i], m2[i], ta, tb);
                        }
                    } else {
                        // branch-free: the other chain gets zero terms (masked d); the tail
                        // chain first (unit k's pixels 0-3, then unit k+1's, in order)
#pragma unroll
                        for (int u = 0; u < 2; u++) {
                            const unsigned *xp = XP[k + u], *yp = YP[k + u];
                            const int nm = ~ms[u];
                            int a0 = mad16<0>(d[u][0] & nm, xp[0], T1[4]);
                            int a1 = mad16<1>(d[u][1] & nm, xp[0], a0);
                            run2(T1[4], M1[4], m1[4], a0, a1);
                            a0 = mad16<0>(d[u][2] & nm, xp[1], T1[4]);
                            a1 = mad16<1>(d[u][3] & nm, xp[1], a0);
                            run2(T1[4], M1[4], m1[4], a0, a1);
                            a0 = mad16<0>(d[u][0] & nm, yp[0], T2[4]);
                            a1 = mad16<1>(d[u][1] & nm, yp[0], a0);
                            run2(T2[4], M2[4], m2[4], a0, a1);
                            a0 = mad16<0>(d[u][2] & nm, yp[1], T2[4]);
                            a1 = mad16<1>(d[u][3] & nm, yp[1], a0);
                            run2(T2[4], M2[4], m2[4], a0, a1);
                        }
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int h = i >> 1;
                            const int e0 = d[0][i] & ms[0], e1 = d[1][i] & ms[1];
                            int ta, tb;
                            if (i & 1) {
                                ta = mad16<1>(e0, XP[k][h], T1[i]);
                                tb = mad16<1>(e1, XP[k + 1][h], ta);
                            } else {
                                ta = mad16<0>(e0, XP[k][h], T1[i]);
                                tb = mad16<0>(e1, XP[k + 1][h], ta);
                            }
                            run2(T1[i], M1[i], m1[i], ta, tb);
                            if (i & 1) {
                                ta = mad16<1>(e0, YP[k][h], T2[i]);
                                tb = mad16<1>(e1, YP[k + 1][h], ta);
                            } else {
                                ta = mad16<0>(e0, YP[k][h], T2[i]);
                                tb = mad16<0>(e1, YP[k + 1][h], ta);
                            }
                            run2(T2[i], M2[i], m2[i], ta, tb);
                        }
                    }
                    // materialize the runs per unit pair (no sinking across pairs)
                    asm volatile("" : "+v"(T1[0]), "+v"(T1[1]), "+v"(T1[2]), "+v"(T1[3]), "+v"(T1[4]), "+v"(M1[0]),
                                 "+v"(M1[1]), "+v"(M1[2]), "+v"(M1[3]), "+v"(M1[4]));
                    asm volatile("" : "+v"(m1[0]), "+v"(m1[1]), "+v"(m1[2]), "+v"(m1[3]), "+v"(m1[4]), "+v"(T2[0]),
                                 "+v"(T2[1]), "+v"(T2[2]), "+v"(T2[3]), "+v"(T2[4]));
                    asm volatile("" : "+v"(M2[0]), "+v"(M2[1]), "+v"(M2[2]), "+v"(M2[3]), "+v"(M2[4]), "+v"(m2[0]),
                                 "+v"(m2[1]), "+v"(m2[2]), "+v"(m2[3]), "+v"(m2[4]), "+v"(dmx), "+v"(dmn));
                }
            };
            if (dtrack)
                bmain(std::true_type());
            else
                bmain(std::false_type());
            const int dmax = max(dmx, -dmn);
            // masked pixels carry zero gradients but any d: only real terms count
            const bool bad = (long long)dmax * gmax > (long long)kExact;
            int T[10], M[10], m[10];
#pragma unroll
            for (int c = 0; c < 5; c++) {
                T[c] = T1[c], M[c] = M1[c], m[c] = m1[c];
                T[5 + c] = T2[c], M[5 + c] = M2[c], m[5 + c] = m2[c];
            }
            PSN_PH_MARK(bx_acc, bx_t, 4);  // b main pass
            bx_prio_hi();
            int *rec = X + par * 4 * kBxRecInts;
            par ^= 1;
            bx_publish<10>(T, rec, NOTAIL || tB == 0);
            PSN_PH_MARK(bx_acc, bx_t, 9);  // b publish (this wave's scans and records)
            __syncthreads();
            bx_check<10>(T, M, m, bad, rec, NOTAIL || tB == 0);
            __syncthreads();
            int tot, h0, base0;
            float b1, b2;
            const bool bex = bx_eval<10>(rec, tot, h0, base0);
            PSN_PH_MARK(bx_acc, bx_t, 5);  // b publish + barrier + eval
            if (bex) {
                combine_b10([&](int i) { return rl_f(tot, i); }, sse, b1, b2);
            } else {
                // ordered float chains from half wave h0 on, tiles of 32 threads' units,
                // double-buffered: the threads of tile g+1 write its products while the
                // chain lanes (wave 0, lanes 0-9, starting from the exact prefixes
                // base0) sum tile g
                // thread roles from an opaque copy of the thread id (see the A fallback)
                int ftid = (int)threadIdx.x;
                asm volatile("" : "+v"(ftid));
                const int HW = QT ? 1 : Q.bx_hw, PC = bx_pc(UPT, TG) * HW;
                const bool chl = ftid < 10;  // wave 0 (as in the A fallback)
                const int cl = chl ? ftid : 0, cs = cl / 5, cc = cl - 5 * cs;
                float acc = (float)base0;
                const int g_last = (U - 1) / (TG * UPT), g_first = h0 * TPH;
                // (CNT, as the A fallback's) once per fallback: the chain lane's region offset in a full tile
                [[maybe_unused]] const int roff = cs * PF + cc * SF;
                [[maybe_unused]] const bool one = HW == 1;
                // (as the A fallback's geoA_g)
                auto tile_geo_g = [&](int g, int &sa, int &ta, int &nsse, int &ntail, auto shortT) {
                    const int ua = TG * UPT * g, ub = min(ua + TG * UPT * HW, U);
                    if constexpr (NOTAIL && (decltype(shortT)::value || POL::kShortWriterGeo)) {
                        static_assert((TG * UPT) % 16 == 0, "a full no-tail tile has no pad");
                        bx_tile_slots_nt(ua, ub, sa, ta, nsse, ntail);
                    } else {
                        bx_tile_slots(ua, ub, QW, nqB, n8, tB, sa, ta, nsse, ntail);
                    }
                };
                auto tile_geo = [&](int g, int &sa, int &ta, int &nsse, int &ntail) {
                    tile_geo_g(g, sa, ta, nsse, ntail, std::true_type());
                };
                // one unit's b products into the tile's chain regions
                auto tile_unit = [&](int yk, int qk, bool uv, const unsigned (&ip)[2], const unsigned (&xp)[2],
                                     const unsigned (&yp)[2], float *buf, int S, int P, int sa, int ta, int zf) {
                    if (!uv) return;
                    int d[4];
                    bx_diffs(JR32 + (oy + yk) * JRP4 + (ox >> 2) + qk, JRP4, W0, W1, s0, s1, s2, s3, ip, d, zf);
                    const bool su = NOTAIL || qk < nqB;
                    const int base = su ? yk * nqB + qk - sa : 4 * S + yk * tB + 4 * qk - n8 - ta;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        // pixels past the window width write a dummy slot past the buffers (branch-free)
                        const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                        const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                        const bool on = 4 * qk + i < w;
                        float *d1 = on ? buf + (su ? i * S + base : base + i) : PL + 6 * PC;  // past 3 buffers
                        d1[0] = (float)__mul24(d[i], gx);
                        d1[on ? P : 1] = (float)__mul24(d[i], gy);
                    }
                };
                // Half-wave tiles (HW = 1): the whole wave writes one tile, K1 = UPT/2
                // unit slots per lane. v_permlane32_swap of unit registers k and K1 + k
                // gives, as its first result, lower lane l's unit k on lane l and its
                // unit K1 + k on lane l + 32 (a lower-half tile), as its second, upper
                // lane l + 32's unit K1 + k there and its unit k on lane l (an upper-half
                // tile): both halves run one instruction stream.
                constexpr int K1 = UPT / 2;
                const bool split = !QT && HW == 1 && (UPT & 1) == 0;
                auto swp = [](unsigned a, unsigned b, bool first) {
                    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                    return first ? r[0] : r[1];
                };
                // two-wave build, quarter-wave tiles (as the A fallback's writeA_q): the
                // unit pair's packed J offsets travel like its window values
                auto write_tile_q = [&](int g, float *buf, auto tqT) __attribute__((always_inline)) {
                    constexpr int TQ = decltype(tqT)::value;
                    const int zf = opaque256();
                    const unsigned qo0 = (unsigned)((const uint8_t *)(JR32 + oy * JRP4 + (ox >> 2)) - smem);
                    const unsigned qo1 = qo0 + 4u * (unsigned)JRP4;
                    int sa, ta, nsse, ntail;
                    tile_geo(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const int rel = (ftid & 15) * UPT + 2 * ((ftid >> 4) & 3), ub = TG * UPT * g + rel;
                    constexpr int U2 = UPT > 4 ? 2 : 0, U3 = UPT > 6 ? 3 : 0;  // (only this build instantiates the body)
                    const unsigned ubp = bx_qpick<TQ>(UB[0], UB[1], UB[U2], UB[U3]);
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const unsigned ip[2] = {bx_qpick<TQ>(IP[j][0], IP[2 + j][0], IP[4 + j][0], IP[6 + j][0]),
                                                bx_qpick<TQ>(IP[j][1], IP[2 + j][1], IP[4 + j][1], IP[6 + j][1])};
                        const unsigned xp[2] = {bx_qpick<TQ>(XP[j][0], XP[2 + j][0], XP[4 + j][0], XP[6 + j][0]),
                                                bx_qpick<TQ>(XP[j][1], XP[2 + j][1], XP[4 + j][1], XP[6 + j][1])};
                        const unsigned yp[2] = {bx_qpick<TQ>(YP[j][0], YP[2 + j][0], YP[4 + j][0], YP[6 + j][0]),
                                                bx_qpick<TQ>(YP[j][1], YP[2 + j][1], YP[4 + j][1], YP[6 + j][1])};
                        const unsigned off = j ? ubp >> 16 : ubp & 0xffffu;
                        if (ub + j < U) {
                            int d[4];
                            bx_diffs2((const uint32_t *)(smem + qo0 + off), (const uint32_t *)(smem + qo1 + off), W0, W1, s0,
                                      s1, s2, s3, ip, d, zf);
                            // (bx_store_b written out, as writeA_q's store)
                            float *d1 = buf + rel + j;
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                                const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                                d1[i * S] = (float)__mul24(d[i], gx);
                                d1[i * S + P] = (float)__mul24(d[i], gy);
                            }
                        }
                    }
                };
                auto write_tile_qt = [&](int g, float *buf, auto) __attribute__((always_inline)) {
                    if ((ftid >> 6) != (g >> 2)) return;
                    switch (g & 3) {
                        case 0: write_tile_q(g, buf, std::integral_constant<int, 0>()); break;
                        case 1: write_tile_q(g, buf, std::integral_constant<int, 1>()); break;
                        case 2: write_tile_q(g, buf, std::integral_constant<int, 2>()); break;
                        default: write_tile_q(g, buf, std::integral_constant<int, 3>()); break;
                    }
                };
                auto write_tile = [&](int g, float *buf) {
                    const int zf = opaque256();  // per tile: no diff constants hoisted out of the tile loop
                    int sa, ta, nsse, ntail;
                    if (split) {
                        if ((ftid >> 6) != (g >> 1)) return;
                        tile_geo(g, sa, ta, nsse, ntail);
                        const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                        const bool lower = (g & 1) == 0, own = ((ftid >> 5) & 1) == (g & 1);
                        const int ub = (own ? ftid : ftid ^ 32) * UPT + (lower == own ? 0 : K1);
                        int yk = ub / QW, qk = ub - yk * QW;
                        asm volatile("" : "+v"(yk), "+v"(qk));
#pragma unroll
                        for (int k = 0; k < K1; k++) {
                            const unsigned ip[2] = {swp(IP[k][0], IP[K1 + k][0], lower), swp(IP[k][1], IP[K1 + k][1], lower)};
                            const unsigned xp[2] = {swp(XP[k][0], XP[K1 + k][0], lower), swp(XP[k][1], XP[K1 + k][1], lower)};
                            const unsigned yp[2] = {swp(YP[k][0], YP[K1 + k][0], lower), swp(YP[k][1], YP[K1 + k][1], lower)};
                            tile_unit(yk, qk, ub + k < U, ip, xp, yp, buf, S, P, sa, ta, zf);
                            if (++qk == QW) {
                                qk = 0;
                                yk++;
                            }
                        }
                        return;
                    }
                    if ((ftid >> 5) < g || (ftid >> 5) >= g + HW) return;
                    tile_geo(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    if constexpr (NOTAIL && UPT <= 8) {  // the thread's own units: offsets from UB, slots from their index
                        unsigned fo0 = (unsigned)((const uint8_t *)(JR32 + oy * JRP4 + (ox >> 2)) - smem);
                        unsigned fo1 = fo0 + 4u * (unsigned)JRP4;
                        asm volatile("" : "+s"(fo0), "+s"(fo1));
                        const int rel = u0 - 32 * UPT * g;
#pragma unroll
                        for (int k = 0; k < UPT; k++) {
                            if (u0 + k >= U) break;
                            // opaque copies: nothing of the unit is hoisted out of the tile loop
                            unsigned ubk = UB[k >> 1], ip[2] = {IP[k][0], IP[k][1]}, xp[2] = {XP[k][0], XP[k][1]},
                                     yp[2] = {YP[k][0], YP[k][1]};
                            asm volatile("" : "+v"(ubk), "+v"(ip[0]), "+v"(ip[1]), "+v"(xp[0]), "+v"(xp[1]), "+v"(yp[0]),
                                         "+v"(yp[1]));
                            const unsigned off = (k & 1) ? ubk >> 16 : ubk & 0xffffu;
                            int d[4];
                            bx_diffs2((const uint32_t *)(smem + fo0 + off), (const uint32_t *)(smem + fo1 + off), W0, W1, s0,
                                      s1, s2, s3, ip, d, zf);
                            bx_store_b(buf + rel + k, d, xp, yp, S, P);
                        }
                        return;
                    }
                    int yk = y0, qk = q0;
                    asm volatile("" : "+v"(yk), "+v"(qk));
#pragma unroll
                    for (int k = 0; k < UPT; k++) {
                        tile_unit(yk, qk, u0 + k < U, IP[k], XP[k], YP[k], buf, S, P, sa, ta, zf);
                        if (++qk == QW) {
                            qk = 0;
                            yk++;
                        }
                    }
                };
                // No-tail build, half-wave tiles: the unit's J dwords from its packed
                // offset (UB, swapped like the window values) and its plane slot from its
                // index in the tile (every quad is an SSE2 quad, every pixel inside the
                // window); the tile's half picked at compile time (no select per value)
                unsigned fo0 = (unsigned)((const uint8_t *)(JR32 + oy * JRP4 + (ox >> 2)) - smem);
                if constexpr (QT) fo0 = (unsigned)__builtin_amdgcn_readfirstlane((int)fo0);
                unsigned fo1 = fo0 + 4u * (unsigned)JRP4;
                asm volatile("" : "+s"(fo0), "+s"(fo1));
                auto write_tile_nt = [&](int g, float *buf, auto lowerT) {
                    constexpr bool lower = decltype(lowerT)::value;
                    const int zf = opaque256();
                    int sa, ta, nsse, ntail;
                    tile_geo_g(g, sa, ta, nsse, ntail, std::false_type());  // (the general form: see geoA_g)
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const bool up = (ftid & 32) != 0;
                    // lower tile: lane l < 32 its unit k, lane l + 32 lane l's unit K1 + k;
                    // upper tile: lane l < 32 lane l + 32's unit k, lane l + 32 its unit K1 + k
                    const int ub = lower ? (up ? (ftid ^ 32) * UPT + K1 : ftid * UPT) : (up ? ftid * UPT + K1 : (ftid ^ 32) * UPT);
                    const int rel = ub - 32 * UPT * g;
                    auto pick = [](unsigned a, unsigned b) {
                        auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                        return lower ? r[0] : r[1];
                    };
                    auto uoff = [&](int k) { return (k & 1) ? UB[k >> 1] >> 16 : UB[k >> 1] & 0xffffu; };
#pragma unroll
                    for (int k = 0; k < K1; k++) {
                        const unsigned ip[2] = {pick(IP[k][0], IP[K1 + k][0]), pick(IP[k][1], IP[K1 + k][1])};
                        const unsigned xp[2] = {pick(XP[k][0], XP[K1 + k][0]), pick(XP[k][1], XP[K1 + k][1])};
                        const unsigned yp[2] = {pick(YP[k][0], YP[K1 + k][0]), pick(YP[k][1], YP[K1 + k][1])};
                        const unsigned off = pick(uoff(k), uoff(K1 + k));
                        if (ub + k < U) {
                            int d[4];
                            bx_diffs2((const uint32_t *)(smem + fo0 + off), (const uint32_t *)(smem + fo1 + off), W0, W1, s0,
                                      s1, s2, s3, ip, d, zf);
                            // (bx_store_b written out: through the helper <16, true> takes one VGPR more)
                            float *d1 = buf + rel + k;
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const int gx = (i & 1) ? hi16(xp[i >> 1]) : lo16(xp[i >> 1]);
                                const int gy = (i & 1) ? hi16(yp[i >> 1]) : lo16(yp[i >> 1]);
                                d1[i * S] = (float)__mul24(d[i], gx);
                                d1[i * S + P] = (float)__mul24(d[i], gy);
                            }
                        }
                    }
                };
                auto pad_tile = [&](int g, float *buf) {  // chain lanes: zero their region's pad
                    if (!chl) return;
                    int sa, ta, nsse, ntail;
                    tile_geo(g, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const int len = cc < 4 ? nsse : ntail;
                    float *rg = buf + cs * P + cc * S;
                    for (int i = len; i < ((len + 15) & ~15); i++) rg[i] = 0.f;
                };
                if (split) {
                    // Three tile buffers, handed over through LDS flags instead of a
                    // workgroup barrier per tile: wave w writes its tiles 2w, 2w+1 as
                    // soon as their buffers are free (tile g waits for the chain lanes
                    // to finish tile g - 3), wave 0 first writes its own tiles, then
                    // its chain lanes sum tile after tile as each one is flagged ready.
                    // No cycle: tile g's writer waits only for tiles of lower waves.
                    const int ep = ++fb_epoch, wv = ftid >> 6, fl = ftid & 63;
                    auto tag = [&](int g) { return ep * 16 + g; };
                    auto spin = [&](int idx, int want) {
                        for (int n = 0; n < (1 << 22); n++) {  // (a bound: never a hang)
                            if (__builtin_amdgcn_readfirstlane(FLG[idx]) == want) break;
                            __builtin_amdgcn_s_sleep(1);
                        }
                        // the bound ran out: the tile may be half written, fail the point
                        if (__builtin_amdgcn_readfirstlane(FLG[idx]) != want) FLG[6] = 1;
                        asm volatile("" ::: "memory");
                    };
                    for (int g = max(h0, 2 * wv); g <= min(2 * wv + 1, g_last); g++) {
                        const int b = (g - h0) % 3;
                        if (g - h0 >= 3) spin(3 + b, tag(g - 3));
                        if constexpr (NOTAIL) {
                            if (g & 1)
                                write_tile_nt(g, PL + b * 2 * PC, std::false_type());
                            else
                                write_tile_nt(g, PL + b * 2 * PC, std::true_type());
                        } else {
                            write_tile(g, PL + b * 2 * PC);
                        }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        if (fl == 0) FLG[b] = tag(g);
                    }
                    PSN_PH_MARK(bx_acc, bx_t, 6);  // serial b: own tiles' products
                    if (wv == 0) {
                        for (int g = h0; g <= g_last; g++) {
                            const int b = (g - h0) % 3;
#ifdef PSN_LK_STAMPS
                            unsigned long long tf0, tf1, tf2, tf3, tf4;
                            PSN_CLK_ORDERED(tf0);
#endif
                            spin(b, tag(g));
                            PSN_CLK_ORDERED(tf1);
                            float *cur = PL + b * 2 * PC;
                            bool full = false;  // (CNT) a full tile (split: one granule per tile) has no pad
                            if constexpr (CNT) full = TG * UPT * (g + 1) <= U;
                            if constexpr (CNT) {
                                if (full) {
                                    PSN_CLK_ORDERED(tf2);
                                    if (chl && cc < 4) acc = chain_sum_nt<NBF>(cur + roff, acc PSN_STAMPS_ONLY(, &bx_tl[30 - 19]));
                                    PSN_CLK_ORDERED(tf3);
                                }
                            }
                            if (!full) {
                            int sa, ta, nsse, ntail;
                            tile_geo(g, sa, ta, nsse, ntail);
                            const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                            const int len = chl ? (cc < 4 ? nsse : ntail) : 0;
                            if (chl) {  // zero this chain's pad (its writer never touches it)
                                float *rg = cur + cs * P + cc * S;
                                for (int i = len; i < ((len + 15) & ~15); i++) rg[i] = 0.f;
                            }
                            const int nbmax = NOTAIL ? (nsse + 15) >> 4 : __builtin_amdgcn_readlane(wave_max_scan((len + 15) >> 4), 63);
                            PSN_CLK_ORDERED(tf2);
                            if (chl && (!NOTAIL || cc < 4))
                                acc = chain_sum_pl<NOTAIL>(cur + cs * P + cc * S, len, nbmax, acc PSN_STAMPS_ONLY(, &bx_tl[30 - 19]));
                            PSN_CLK_ORDERED(tf3);
                            }
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            if (fl == 0) FLG[3 + b] = tag(g);
#ifdef PSN_LK_STAMPS
                            PSN_CLK_ORDERED(tf4);
                            BX_TL(25, tf1 - tf0);                  // wait for the tile's ready flag
                            BX_TL(26, (tf2 - tf1) + (tf4 - tf3));  // geometry + pad + the consumed flag
                            BX_TL(27, tf3 - tf2);                  // chain sums (first-block wait: 30)
                            BX_TL(28, 1);
                            if (g == h0) {  // of 25 and 28: the first tile of a fallback pass
                                BX_TL(31, tf1 - tf0);
                                BX_TL(32, 1);
                            }
#endif
                        }
                    }
                } else {
                if constexpr (QT)
                    write_tile_qt(g_first, PL, 0);
                else
                    write_tile(g_first, PL);
                pad_tile(g_first, PL);
                __syncthreads();
                PSN_PH_MARK(bx_acc, bx_t, 6);  // serial b: first tile's products
                for (int g = g_first, t = 0; g <= g_last; g += HW, t ^= 1) {  // tile = granules g .. g+HW-1
                    float *cur = PL + t * 2 * PC, *nxt = PL + (t ^ 1) * 2 * PC;
                    if (g + HW <= g_last) {
                        if constexpr (QT)
                            write_tile_qt(g + HW, nxt, 0);
                        else
                            write_tile(g + HW, nxt);
                    }
#ifdef PSN_LK_STAMPS
                    unsigned long long tc0, tc1, tc2, tc3, tc4;
                    PSN_CLK_ORDERED(tc0);
                    tc3 = tc4 = tc0;
#endif
                    bool full = false;  // (CNT) the straight-line step of a full tile
                    if constexpr (CNT) full = one && TG * UPT * (g + 1) <= U;
                    if constexpr (CNT) {
                        if (full && (ftid >> 6) == 0) {
                            PSN_CLK_ORDERED(tc3);
                            if (chl && cc < 4) acc = chain_sum_nt<NBF>(cur + roff, acc PSN_STAMPS_ONLY(, &bx_tl[30 - 19]));
                            PSN_CLK_ORDERED(tc4);
                            // only the window's last tile can have a pad
                            if (g + 1 == g_last) pad_tile(g_last, nxt);
                        }
                    }
                    if (!full && (ftid >> 6) == 0) {
                        int sa, ta, nsse, ntail;
                        tile_geo(g, sa, ta, nsse, ntail);
                        const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                        const int len = chl ? (cc < 4 ? nsse : ntail) : 0;
                        // (no-tail: every chain lane's length is nsse)
                        const int nbmax = NOTAIL ? (nsse + 15) >> 4 : __builtin_amdgcn_readlane(wave_max_scan((len + 15) >> 4), 63);
                        PSN_CLK_ORDERED(tc3);
                        // (no-tail: the tail-chain lanes keep acc = 0)
                        if (chl && (!NOTAIL || cc < 4))
                            acc = chain_sum_pl<NOTAIL>(cur + cs * P + cc * S, len, nbmax, acc PSN_STAMPS_ONLY(, &bx_tl[30 - 19]));
                        PSN_CLK_ORDERED(tc4);
                        if (g + HW <= g_last) pad_tile(g + HW, nxt);
                    }
#ifdef PSN_LK_STAMPS
                    PSN_CLK_ORDERED(tc1);
#endif
                    __syncthreads();
#ifdef PSN_LK_STAMPS
                    PSN_CLK_ORDERED(tc2);
                    bx_acc[12] += tc1 - tc0;  // (chain lane 0's view) geometry + chain sums + pad
                    BX_TL(29, tc4 - tc3);     // of it: the chain sums alone (first-block wait: 30)
                    bx_acc[13] += tc2 - tc1;  // barrier wait
                    bx_acc[14]++;
#endif
                }
                }
                PSN_PH_MARK(bx_acc, bx_t, 7);  // serial b: pipelined products + chains
                PSN_PH_COUNT(bx_acc, 11);
                if (ftid < 64) {  // wave 0 combines in the SSE2 build's order
                    float r1, r2;
                    combine_b10([&](int i) { return readlane_f(acc, i); }, sse, r1, r2);
                    if (ftid == 0) {
                        RS[4] = r1;
                        RS[5] = r2;
                    }
                }
                __syncthreads();
                b1 = RS[4];
                b2 = RS[5];
            }
            PSN_PH_MARK(bx_acc, bx_t, 8);  // b results
            float dx, dy;
            const double dd = lk_update(S.A11, S.A12, S.A22, S.invD, b1, b2, hwx, hwy, nx, ny, NPx, NPy, dx, dy);
            if (lk_stop(dd, Q.eps2, j, dx, dy, pdx, pdy, NPx, NPy)) break;
        }

        if (level == 0 && status && A.err && (flags & PSN_LK_GET_MIN_EIGENVALS) == 0) {
            const float qx = __fsub_rn(NPx, hwx), qy = __fsub_rn(NPy, hwy);
            const int iqx = cv_floor(qx), iqy = cv_floor(qy);
            if (win_outside(iqx, iqy, w, h, cols, rows)) {
                status = 0;
                continue;
            }
            // PSN_LK_ERR_STATUS_ONLY: the re-check above was all of err the caller
            // wanted (err[] = 0); the builds held to their register counts ignore it
            if constexpr (POL::kErrStatusOnly || QT)
                if (flags & PSN_LK_ERR_STATUS_ONLY) continue;
            PSN_CLK_ORDERED(bx_te);  // stamp 33: the err pass (from here to the level's end)
            int w00, w01, w10, w11;
            bilin_weights(__fsub_rn(qx, (float)iqx), __fsub_rn(qy, (float)iqy), w00, w01, w10, w11);
            if (!(jr_covers(iqx, iqy, w, h, jr_x0, jr_y0, JRW, JRH))) {
                __syncthreads();  // a serial b pass may still read nothing of JR, but be safe
                jr_x0 = (iqx - kStJMargin) & ~3;
                jr_y0 = iqy - kStJMargin;
                dma_patch<NT>(JR, J, jr_y0, jr_x0, JRW, JRH, JRP4, Q.dv_bxjr);
                dma_wait();
                __syncthreads();
            }
            const unsigned W0 = pack_w(w00, w01), W1 = pack_w(w10, w11);
            const int ox = iqx - jr_x0, oy = iqy - jr_y0, sj = ox & 3;
            const unsigned s0 = bx_sel(sj, 0), s1 = bx_sel(sj, 1), s2 = bx_sel(sj, 2), s3 = bx_sel(sj, 3);
            unsigned e = 0;
            {
                int y = y0, q = q0;
            asm volatile("" : "+v"(y), "+v"(q));  // opaque: no per-unit address hoisting (VGPRs)
#pragma unroll
                for (int k = 0; k < UPT; k++) {
                    const bool uv = u0 + k < U;
                    int d[4];
                    bx_diffs(JR32 + (oy + (uv ? y : 0)) * JRP4 + (ox >> 2) + (uv ? q : 0), JRP4, W0, W1, s0, s1, s2, s3, IP[k], d, 256);
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (uv && 4 * q + i < w) e += (unsigned)abs(d[i]);
                    if (++q == QW) {
                        q = 0;
                        y++;
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one unit at a time (register pressure)
                }
            }
            e = (unsigned)wave_sum((int)e);  // <= 64 * 48 * 8160 < 2^31
            if (lane == 0) EP[tid >> 6] = (int)e;
            __syncthreads();
            unsigned et = 0;
#pragma unroll
            for (int wv = 0; wv < NW; wv++) et += (unsigned)EP[wv];
            float errval;
            if (et <= (unsigned)kExact) {
                errval = (float)et;  // every partial sum of errval += |diff| is an exact integer
            } else {  // row-major order, one lane, row tiles
                const int TR = Q.bx_tre;
                float acc = 0.f;
                for (int r0 = 0; r0 < h; r0 += TR) {
                    const int tr = min(TR, h - r0);
                    __syncthreads();
                    int yk = y0, qk = q0;
                    asm volatile("" : "+v"(yk), "+v"(qk));
#pragma unroll
                    for (int k = 0; k < UPT; k++) {
                        if (u0 + k < U && yk >= r0 && yk < r0 + tr) {
                            int d[4];
                            bx_diffs(JR32 + (oy + (yk)) * JRP4 + (ox >> 2) + (qk), JRP4, W0, W1, s0, s1, s2, s3, IP[k], d, 256);
#pragma unroll
                            for (int i = 0; i < 4; i++)
                                if (4 * qk + i < w) PL[(yk - r0) * w + 4 * qk + i] = (float)abs(d[i]);
                        }
                        if (++qk == QW) {
                            qk = 0;
                            yk++;
                        }
                    }
                    __syncthreads();
                    if (tid == 0) acc = chain_sum(PL, tr * w, acc);
                }
                if (tid == 0) RS[8] = acc;
                __syncthreads();
                errval = RS[8];
            }
            errv = lk_err(errval, w * h);
        }
    }

#ifdef PSN_LK_STAMPS
    {
        unsigned long long t_end;
        PSN_CLK_ORDERED(t_end);
        bx_acc[15] = t_end - bx_t0;
        if (bx_te) bx_te = t_end - bx_te;  // (level 0 is the last level: the pass ends here)
        unsigned long long r1;
        unsigned hwid, xcc;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1) : : "memory");
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if (tid == 0 && A.stamps) {  // thread 0: also the chain lane of the tile stamps 12-14
            for (int i = 0; i < 16; i++) A.stamps[(size_t)g * 64 + i] = bx_acc[i];
            for (int i = 19; i < 33; i++) A.stamps[(size_t)g * 64 + i] = bx_tl[i - 19];  // fallback tile splits
            A.stamps[(size_t)g * 64 + 33] = bx_te;  // the err pass (0: not run)
            // residency: realtime (100 MHz) start / end and the CU it ran on
            A.stamps[(size_t)g * 64 + 16] = bx_r0;
            A.stamps[(size_t)g * 64 + 17] = r1;
            A.stamps[(size_t)g * 64 + 18] = ((unsigned long long)xcc << 32) | hwid;
        }
    }
#endif
#ifdef PSN_LK_STAMPS
#undef BX_TL
#endif
    if (tid == 0) {
        if (FLG[6]) {  // a fallback hand-off timed out: the sums may be wrong -- say so
            NPx = NPy = errv = __builtin_nanf("");
            status = 0;
        }
        A.next[2 * pi] = NPx;
        A.next[2 * pi + 1] = NPy;
        A.status[pi] = (uint8_t)status;
        if (A.err) A.err[pi] = errv;
        if (A.samples) atomicAdd(A.samples, (unsigned long long)nwin * (unsigned)(w * h));
    }
