// The body of k_batch_riccati (eqf_batch.hpp), included once per kernel, as eqf_batch_frame_body.inc is: with EQF_BATCH_NORMAL 0 the text k_batch_riccati has
// always had, so that it compiles to the code it has always had; with EQF_BATCH_NORMAL 1 k_batch_riccati_normal, the same samples for the Normal slots
// (eqf_batch.hpp, "The Normal chart"). `ra` is the kernel's RicArgs, `nrm` the Normal kernel's BatchNormalIn array.
    __shared__ double sm[RIC_SM];
    __shared__ double s_red[BATCH_T / 64];
    __shared__ double s_qp[20]; // Q / dt and dt P of the sample
    __shared__ int s_gidx[BATCH_NMAX];
    __shared__ int s_surv[BATCH_L];
    const BatchIn& in = ra.in[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int L = BATCH_L, ld = ra.buf.ld;
#if EQF_BATCH_NORMAL
    const int chart = EQVIO_COORD_EUCLIDEAN; // the samples run in Euclidean coordinates
#else
    const int chart = in.ss.chart;
#endif
    const bool ind = chart == EQVIO_COORD_INVDEPTH;
    const int slot = in.slot, cur = in.cur, nxt = cur ^ 1;
    const double* S0 = ra.buf.sig_of(slot, cur);
    double* S1 = ra.buf.sig_of(slot, nxt);
    const double* L0 = ra.buf.lm_of(slot, cur);
    double* L1 = ra.buf.lm_of(slot, nxt);
    double* G = ra.buf.scr_of(slot);
    const int Ns = in.Ns, n1 = 21 + 3 * Ns, K = in.k;
    double* sP = sm;              // [A B] of the sensor rows (21 x 33, row-major), then scaled
    double* sE = sP + RIC_EN;     // E
    double* sT = sE + RIC_EN;     // the series' current term; afterwards the waves' staging rows (3 x 33 each)
    double* sN = sT + RIC_EN;     // the next term, the next square
    double* lm66 = sN + RIC_EN;
    double* YF = lm66 + 66;       // per landmark: Y (3 x 33, row-major), F (3 x 3)

    for (int t = tid; t < Ns; t += BATCH_T)
        s_surv[t] = in.surv[t];
    __syncthreads();
    for (int r = tid; r < n1; r += BATCH_T)
        s_gidx[r] = r < 21 ? r : 21 + 3 * s_surv[(r - 21) / 3] + (r - 21) % 3;
    // the surviving landmarks' planes into the other buffer; wave 3 keeps (q, a) of its landmark and takes it through the observer steps
    V3 p0{};
    Qt q{};
    double a = 1.0;
    if (wave == 3 && lane < Ns) {
        const int o = s_surv[lane];
        for (int pl = 0; pl < BATCH_PLANES; ++pl)
            L1[pl * L + lane] = L0[pl * L + o];
        p0 = ld3(L0, L, o);
        q = ldq(L0 + BATCH_QQ * L, L, o);
        a = L0[BATCH_QA * L + o];
    }
    __syncthreads();

    bool first = true; // Sigma is still the current buffer's, to be gathered
    int samples = 0, max_sq = 0;
#if EQF_BATCH_NORMAL
    double* pe = G + (size_t)ld * BATCH_NMAX; // M^-1 P M^-T, in the statistics rows of the scratch area
    {
        bool any = false;
        for (int s = 0; s < K; ++s)
            any = any || ra.rsteps[in.obs_off + s].dt > 0.0;
        if (any) {
            const NormalM& nm = nrm[blockIdx.x].inv;
            batch_normal_tables(L1, nullptr, Ns, sm, sm + 9 * BATCH_L);
            __syncthreads();
            batch_normal_noise(nm, sm + 9 * BATCH_L, Ns, in.ss.Pd, pe);
            batch_normal_congruence(nm, sm + 9 * BATCH_L, n1, ld, S0, s_gidx, S1);
            __syncthreads();
            for (int r = tid; r < n1; r += BATCH_T)
                s_gidx[r] = r;
            first = false;
            __syncthreads();
        }
    }
#endif
    for (int s = 0; s < K; ++s) {
        const RicStep& rs = ra.rsteps[in.obs_off + s];
        const double dt = rs.dt;
        if (dt > 0.0) {
            // ---- A and B at this sample's X: the sensor rows into sP, the landmarks' rows into their slots (assemble_landmark<PART>, a wave per column part)
            for (int t = tid; t < RIC_EN; t += BATCH_T) {
                const int r = t / 33, c = t % 33;
                sP[t] = c < 21 ? sensor_Ass_entry(rs.ck, r * 21 + c) : sensor_Bs_entry(rs.ck, r * 12 + (c - 21));
            }
            for (int t = tid; t < 66; t += BATCH_T)
                lm66[t] = rs.ck.lm[t];
            if (tid < 12)
                s_qp[tid] = in.ss.Qd[tid] / dt;
            else if (tid < 20)
                s_qp[tid] = dt * in.ss.Pd[tid - 12];
            __syncthreads();
            if (wave < 3 && lane < Ns) {
                const int i = lane;
                const V3 pi = ld3(L1, L, i);
                const Qt qi = ldq(L1 + BATCH_QQ * L, L, i);
                const double ai = L1[BATCH_QA * L + i];
                const M3 e2i = ind ? ld_cc(L1, L, i, CC_E2I) : M3{}, i2e = ind && wave == 2 ? ld_cc(L1, L, i, CC_I2E) : M3{};
                double al[45], bl[9];
                double* Al = YF + i * RIC_SLOT;
                if (wave == 0) {
                    assemble_landmark<0>(lm66, chart, pi, qi, ai, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 6; ++c)
                            Al[r * 15 + c] = al[r * 15 + c];
                    for (int e = 0; e < 9; ++e)
                        Al[45 + e] = bl[e];
                } else if (wave == 1) {
                    assemble_landmark<1>(lm66, chart, pi, qi, ai, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 6; c < 12; ++c)
                            Al[r * 15 + c] = al[r * 15 + c];
                } else {
                    assemble_landmark<2>(lm66, chart, pi, qi, ai, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 12; c < 15; ++c)
                            Al[r * 15 + c] = al[r * 15 + c];
                }
            }
            __syncthreads();
            // ---- the scaling: s with |dt [A B]|_inf / 2^s <= 0.25 (k_expm_sensor's rule)
            {
                double mx = 0.0;
                if (tid < 21) {
                    for (int c = 0; c < 33; ++c)
                        mx += fabs(sP[tid * 33 + c]);
                } else if (tid >= 64 && tid - 64 < 3 * Ns) {
                    const int i = (tid - 64) / 3, r = (tid - 64) % 3;
                    const double* Al = YF + i * RIC_SLOT;
                    for (int e = 0; e < 15; ++e)
                        mx += fabs(Al[r * 15 + e]);
                    for (int e = 0; e < 3; ++e)
                        mx += fabs(Al[45 + r * 3 + e]);
                }
                for (int o = 32; o > 0; o >>= 1)
                    mx = fmax(mx, __shfl_xor(mx, o, 64));
                if (lane == 0)
                    s_red[wave] = mx;
            }
            __syncthreads();
            int sc = 0;
            {
                const double nrm = dt * fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
                while (sc < EXPM_SMAX && ldexp(nrm, -sc) > 0.25)
                    ++sc;
            }
            const double scale = ldexp(dt, -sc);
            ++samples;
            max_sq = max(max_sq, sc);
            // ---- sensor part: E = sum_k Ps^k / k! (rows 21 .. 32 of Ps are zero: the inner index runs over 21)
            for (int t = tid; t < RIC_EN; t += BATCH_T) {
                const double v = scale * sP[t];
                sP[t] = v;
                sT[t] = v;
                sE[t] = v + (t / 33 == t % 33 ? 1.0 : 0.0);
            }
            __syncthreads();
            for (int k = 2; k <= EXPM_K; ++k) {
                for (int t = tid; t < RIC_EN; t += BATCH_T) {
                    const int r = t / 33, c = t % 33;
                    double acc = 0.0;
                    for (int qq = 0; qq < 21; ++qq)
                        acc += sT[r * 33 + qq] * sP[qq * 33 + c];
                    sN[t] = acc / k;
                }
                __syncthreads();
                for (int t = tid; t < RIC_EN; t += BATCH_T) {
                    sT[t] = sN[t];
                    sE[t] += sN[t];
                }
                __syncthreads();
            }
            // ---- landmark part, a wave per landmark and a lane per column: term_k = (term_{k-1} Ps + S^(k-1) / (k-1)! R) / k (k_expm_landmarks)
            {
                double* sR = sT + wave * 99;
                const int c = lane;
                for (int i = wave; i < Ns; i += BATCH_T / 64) {
                    double* sl = YF + i * RIC_SLOT;
                    double R[3] = {0, 0, 0};
                    if (c < 33) {
                        const int e = c < 3 ? c : (c >= 12 && c < 15) ? 3 + (c - 12) : (c >= 15 && c < 21) ? 6 + (c - 15) : -1;
                        for (int r = 0; r < 3; ++r) {
                            if (e >= 0)
                                R[r] = scale * sl[r * 15 + e];
                            else if (c >= 21 && c < 24)
                                R[r] = scale * sl[45 + r * 3 + (c - 21)];
                        }
                    }
                    double S[9], F[9], Spow[9];
                    for (int r = 0; r < 3; ++r)
                        for (int qq = 0; qq < 3; ++qq) {
                            S[r * 3 + qq] = scale * sl[r * 15 + 12 + qq];
                            Spow[r * 3 + qq] = S[r * 3 + qq];
                            F[r * 3 + qq] = (r == qq ? 1.0 : 0.0) + S[r * 3 + qq];
                        }
                    double T[3] = {R[0], R[1], R[2]}, Y[3] = {R[0], R[1], R[2]};
                    for (int k = 2; k <= EXPM_K; ++k) {
                        batch_wave_sync(); // the staging rows' readers of the round before (and the slot's, before the first one) are done
                        if (c < 33)
                            for (int r = 0; r < 3; ++r)
                                sR[r * 33 + c] = T[r];
                        batch_wave_sync();
                        double nt[3] = {0, 0, 0};
                        if (c < 33) {
                            for (int qq = 0; qq < 21; ++qq) {
                                const double pv = sP[qq * 33 + c];
                                nt[0] += sR[qq] * pv;
                                nt[1] += sR[33 + qq] * pv;
                                nt[2] += sR[66 + qq] * pv;
                            }
                            for (int r = 0; r < 3; ++r)
                                nt[r] = (nt[r] + Spow[r * 3 + 0] * R[0] + Spow[r * 3 + 1] * R[1] + Spow[r * 3 + 2] * R[2]) / k;
                        }
                        double ns[9];
                        for (int r = 0; r < 3; ++r)
                            for (int qq = 0; qq < 3; ++qq)
                                ns[r * 3 + qq] = (Spow[r * 3 + 0] * S[0 * 3 + qq] + Spow[r * 3 + 1] * S[1 * 3 + qq] + Spow[r * 3 + 2] * S[2 * 3 + qq]) / k;
                        for (int r = 0; r < 3; ++r) {
                            T[r] = nt[r];
                            Y[r] += nt[r];
                        }
                        for (int e = 0; e < 9; ++e) {
                            Spow[e] = ns[e];
                            F[e] += ns[e];
                        }
                    }
                    batch_wave_sync();
                    if (c < 33)
                        for (int r = 0; r < 3; ++r)
                            sl[r * 33 + c] = Y[r];
                    if (c < 9)
                        sl[99 + c] = F[c];
                }
            }
            __syncthreads();
            // ---- squarings, in lockstep: Y <- Y E + F Y and F <- F F of every landmark with this round's E, then E <- E E (rows 21 .. 32 of E are [0 I])
            for (int j = 0; j < sc; ++j) {
                const int c = lane;
                for (int i = wave; i < Ns; i += BATCH_T / 64) {
                    double* sl = YF + i * RIC_SLOT;
                    double ny[3] = {0, 0, 0}, nf = 0.0;
                    if (c < 33) {
                        for (int r = 0; r < 3; ++r)
                            ny[r] = c >= 21 ? sl[r * 33 + c] : 0.0;
                        for (int qq = 0; qq < 21; ++qq) {
                            const double pv = sE[qq * 33 + c];
                            ny[0] += sl[qq] * pv;
                            ny[1] += sl[33 + qq] * pv;
                            ny[2] += sl[66 + qq] * pv;
                        }
                        const double y0 = sl[c], y1 = sl[33 + c], y2 = sl[66 + c];
                        for (int r = 0; r < 3; ++r)
                            ny[r] += sl[99 + r * 3 + 0] * y0 + sl[99 + r * 3 + 1] * y1 + sl[99 + r * 3 + 2] * y2;
                    }
                    if (c < 9) {
                        const int r = c / 3, qq = c % 3;
                        nf = sl[99 + r * 3 + 0] * sl[99 + 0 * 3 + qq] + sl[99 + r * 3 + 1] * sl[99 + 1 * 3 + qq] + sl[99 + r * 3 + 2] * sl[99 + 2 * 3 + qq];
                    }
                    batch_wave_sync();
                    if (c < 33)
                        for (int r = 0; r < 3; ++r)
                            sl[r * 33 + c] = ny[r];
                    if (c < 9)
                        sl[99 + c] = nf;
                }
                for (int t = tid; t < RIC_EN; t += BATCH_T) {
                    const int r = t / 33, cc = t % 33;
                    double acc = cc >= 21 ? sE[r * 33 + cc] : 0.0;
                    for (int qq = 0; qq < 21; ++qq)
                        acc += sE[r * 33 + qq] * sE[qq * 33 + cc];
                    sN[t] = acc;
                }
                __syncthreads();
                for (int t = tid; t < RIC_EN; t += BATCH_T)
                    sE[t] = sN[t];
                __syncthreads();
            }
            // ---- Sigma' = Phi Sigma Phi^T + Phi_B (Q / dt) Phi_B^T + dt P
            // row r of Phi applied to a vector given entry by entry (the shape of k_batch_frame's f_row; a landmark row carries all 21 sensor columns)
            auto phi_row = [&](int r, auto v) -> double {
                double acc = 0.0;
                if (r < 21) {
                    for (int k = 0; k < 21; ++k)
                        acc += sE[r * 33 + k] * v(k);
                } else {
                    const int i = (r - 21) / 3, aa = (r - 21) % 3;
                    const double* sl = YF + i * RIC_SLOT;
                    for (int k = 0; k < 21; ++k)
                        acc += sl[aa * 33 + k] * v(k);
                    for (int b = 0; b < 3; ++b)
                        acc += sl[99 + aa * 3 + b] * v(21 + 3 * i + b);
                }
                return acc;
            };
            auto phib = [&](int r, int e) -> double { return r < 21 ? sE[r * 33 + 21 + e] : YF[((r - 21) / 3) * RIC_SLOT + ((r - 21) % 3) * 33 + 21 + e]; };
            const double* Ssrc = first ? S0 : S1;
            for (int t = tid; t < n1 * n1; t += BATCH_T) {
                const int r = t % n1, c = t / n1;
                const double* col = Ssrc + (size_t)s_gidx[c] * ld;
                G[r + (size_t)c * ld] = phi_row(r, [&](int k) { return col[s_gidx[k]]; });
            }
            __syncthreads();
            for (int t = tid; t < n1 * n1; t += BATCH_T) {
                const int r = t % n1, c = t / n1;
                if (r < c)
                    continue;
                double v = phi_row(c, [&](int k) { return G[r + (size_t)k * ld]; });
                double nz = 0.0;
                for (int e = 0; e < 12; ++e)
                    nz += phib(r, e) * s_qp[e] * phib(c, e);
                v += nz;
#if EQF_BATCH_NORMAL
                v += dt * batch_normal_noise_at(pe, r, c);
#else
                if (r == c)
                    v += s_qp[12 + (r < 21 ? r / 3 : 7)];
#endif
                S1[r + (size_t)c * ld] = v;
                S1[c + (size_t)r * ld] = v;
            }
            if (first) { // the gathered rows' readers are behind the barrier above; the next reader is behind the sample's last one
                for (int r = tid; r < n1; r += BATCH_T)
                    s_gidx[r] = r;
                first = false;
            }
        }
        // ---- this sample's observer step of the landmarks
        if (wave == 3 && lane < Ns) {
            observer_chain(ra.steps + in.obs_off + s, 1, p0, q, a);
            L1[BATCH_QQ * L + lane] = q.w;
            L1[(BATCH_QQ + 1) * L + lane] = q.x;
            L1[(BATCH_QQ + 2) * L + lane] = q.y;
            L1[(BATCH_QQ + 3) * L + lane] = q.z;
            L1[BATCH_QA * L + lane] = a;
        }
        __syncthreads();
    }
    if (first) // no sample moved Sigma: the gathered Sigma as it is
        for (int t = tid; t < n1 * n1; t += BATCH_T) {
            const int r = t % n1, c = t / n1;
            S1[r + (size_t)c * ld] = S0[s_gidx[r] + (size_t)s_gidx[c] * ld];
        }
#if EQF_BATCH_NORMAL
    if (samples > 0) { // back into Normal coordinates (the loop's last barrier is behind the last sample's stores)
        batch_normal_tables(L1, nullptr, Ns, sm, sm + 9 * BATCH_L);
        __syncthreads();
        batch_normal_congruence(nrm[blockIdx.x].fwd, sm, n1, ld, S1, s_gidx, G);
        __syncthreads();
        for (int t = tid; t < n1 * n1; t += BATCH_T) {
            const int r = t % n1, c = t / n1;
            S1[r + (size_t)c * ld] = G[r + (size_t)c * ld];
        }
    }
#endif
    if (tid == 0) {
        ra.out[blockIdx.x].ric_samples = samples;
        ra.out[blockIdx.x].ric_squarings = max_sq;
    }
