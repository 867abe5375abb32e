// The body of k_batch_discrete (eqf_batch.hpp), included once per kernel, as eqf_batch_frame_body.inc is: with EQF_BATCH_NORMAL 0 the text k_batch_discrete has
// always had, so that it compiles to the code it has always had; with EQF_BATCH_NORMAL 1 k_batch_discrete_normal, the same samples for the Normal slots
// (eqf_batch.hpp, "The Normal chart"). `da` is the kernel's DiscArgs, `nrm` the Normal kernel's BatchNormalIn array.
    __shared__ double sm[DISC_SM];
    __shared__ Pose s_cpc[1 + DISC_NPERT]; // [0] nominal, [1 + 2 j + s]: DiscreteAArgs::cpc's order
    __shared__ double s_qp[20];            // Q and P of the slot
    __shared__ int s_gidx[BATCH_NMAX];
    __shared__ int s_surv[BATCH_L];
    const BatchIn& in = da.in[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int L = BATCH_L, ld = da.buf.ld;
#if EQF_BATCH_NORMAL
    const int chart = EQVIO_COORD_EUCLIDEAN; // A_d,e and B_e: the samples run in Euclidean coordinates
#else
    const int chart = in.ss.chart;
#endif
    const bool ind = chart == EQVIO_COORD_INVDEPTH;
    const int slot = in.slot, cur = in.cur, nxt = cur ^ 1;
    const double* S0 = da.buf.sig_of(slot, cur);
    double* S1 = da.buf.sig_of(slot, nxt);
    const double* L0 = da.buf.lm_of(slot, cur);
    double* L1 = da.buf.lm_of(slot, nxt);
    double* G = da.buf.scr_of(slot);
    const int Ns = in.Ns, n1 = 21 + 3 * Ns, K = in.k;
    double* sA = sm;              // sensor block of A_d, row-major 21 x 21
    double* sB = sA + 441;        // sensor rows of B, row-major 21 x 12
    double* lm66 = sB + 252;
    double* sCol = lm66 + 66;     // the 42 perturbed evaluations' 21-vectors
    double* AL = sCol + DISC_NPERT * 21; // per landmark: rows of A_d (3 x 24, row-major), then B (3 x 3)
    const double h = cbrt(2.220446049250313e-16), ih2 = 1.0 / (2.0 * h);

    for (int t = tid; t < Ns; t += BATCH_T)
        s_surv[t] = in.surv[t];
    if (tid < 12)
        s_qp[tid] = in.ss.Qd[tid];
    else if (tid < 20)
        s_qp[tid] = in.ss.Pd[tid - 12];
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
    int samples = 0;
#if EQF_BATCH_NORMAL
    double* pe = G + (size_t)ld * BATCH_NMAX; // M^-1 P M^-T, in the statistics rows of the scratch area
    {
        bool any = false;
        for (int s = 0; s < K; ++s)
            any = any || da.dsteps[in.obs_off + s].dt > 0.0;
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
        const DiscStep& ds = da.dsteps[in.obs_off + s];
        const double dt = ds.dt;
        if (dt > 0.0) {
            ++samples;
            // ---- a0Discrete's sensor part: the nominal evaluation and the 42 perturbed ones (wave 0); B's sensor rows and the landmark factors (the other waves)
            if (wave == 0) {
                if (lane <= DISC_NPERT)
                    disc_sensor_eval<EQF_BATCH_NORMAL>(ds, lane, h, sCol, s_cpc);
            } else {
                for (int t = tid - 64; t < 252; t += BATCH_T - 64)
                    sB[t] = sensor_Bs_entry(ds.ck, t);
                for (int t = tid - 64; t < 66; t += BATCH_T - 64)
                    lm66[t] = ds.ck.lm[t];
            }
            __syncthreads();
            // ---- the sensor block: the pairs differenced
            for (int t = tid; t < 441; t += BATCH_T) {
                const int r = t / 21, j = t % 21;
                sA[t] = (sCol[(2 * j) * 21 + r] - sCol[(2 * j + 1) * 21 + r]) * ih2;
            }
            // ---- the landmarks' rows: a lane per landmark, six of its 24 central differences per wave; wave 0 also its 3 x 3 of B
            if (lane < Ns) {
                const int i = lane;
                const V3 q0 = ld3(L1, L, i);
                const Sot3 Qi{ldq(L1 + BATCH_QQ * L, L, i), L1[BATCH_QA * L + i]};
                const V3 qh = (1.0 / Qi.a) * q_rot(q_inv(Qi.R), q0);
                const Pose cpc0 = s_cpc[0];
                const Sot3 QLh_inv = sot3_inv(lift_q(cpc0, qh)); // liftVelocityDiscrete(xi_hat)^-1, landmark i
                double* row = AL + i * DISC_SLOT;
#pragma unroll 1
                for (int c = 6 * wave; c < 6 * wave + 6; ++c) {
                    V3 ep, em;
                    if (c < 21) {
                        ep = a0_discrete_landmark(chart, Qi, QLh_inv, s_cpc[1 + 2 * c], q0, q0);
                        em = a0_discrete_landmark(chart, Qi, QLh_inv, s_cpc[2 + 2 * c], q0, q0);
                    } else {
                        const int k = c - 21;
                        const V3 e = V3{k == 0 ? h : 0.0, k == 1 ? h : 0.0, k == 2 ? h : 0.0};
                        ep = a0_discrete_landmark(chart, Qi, QLh_inv, cpc0, chart_bwd(chart, e, q0), q0);
                        em = a0_discrete_landmark(chart, Qi, QLh_inv, cpc0, chart_bwd(chart, -e, q0), q0);
                    }
                    const V3 d = ih2 * (ep - em);
                    row[c] = d.x;
                    row[DISC_ROW + c] = d.y;
                    row[2 * DISC_ROW + c] = d.z;
                }
                if (wave == 0) {
                    const M3 e2i = ind ? ld_cc(L1, L, i, CC_E2I) : M3{};
                    double al[45], bl[9];
                    assemble_landmark<0>(lm66, chart, q0, Qi.R, Qi.a, e2i, M3{}, al, bl);
                    for (int e = 0; e < 9; ++e)
                        row[3 * DISC_ROW + e] = bl[e];
                }
            }
            __syncthreads();
            // ---- Sigma' = A_d Sigma A_d^T + dt (B Q B^T + P)
            // row r of A_d applied to a vector given entry by entry (k_batch_riccati's phi_row)
            auto ad_row = [&](int r, auto v) -> double {
                double acc = 0.0;
                if (r < 21) {
                    for (int k = 0; k < 21; ++k)
                        acc += sA[r * 21 + k] * v(k);
                } else {
                    const int i = (r - 21) / 3, aa = (r - 21) % 3;
                    const double* rw = AL + i * DISC_SLOT + aa * DISC_ROW;
                    for (int k = 0; k < 21; ++k)
                        acc += rw[k] * v(k);
                    for (int b = 0; b < 3; ++b)
                        acc += rw[21 + b] * v(21 + 3 * i + b);
                }
                return acc;
            };
            auto b_entry = [&](int r, int e) -> double {
                if (r < 21)
                    return sB[r * 12 + e];
                return e < 3 ? AL[((r - 21) / 3) * DISC_SLOT + 3 * DISC_ROW + ((r - 21) % 3) * 3 + e] : 0.0;
            };
            if constexpr (!(EQF_DISC_MEASURE_SKIP & 1)) {
                const double* Ssrc = first ? S0 : S1;
                for (int t = tid; t < n1 * n1; t += BATCH_T) {
                    const int r = t % n1, c = t / n1;
                    const double* col = Ssrc + (size_t)s_gidx[c] * ld;
                    G[r + (size_t)c * ld] = ad_row(r, [&](int k) { return col[s_gidx[k]]; });
                }
                __syncthreads();
                for (int t = tid; t < n1 * n1; t += BATCH_T) {
                    const int r = t % n1, c = t / n1;
                    if (r < c)
                        continue;
                    double v = ad_row(c, [&](int k) { return G[r + (size_t)k * ld]; });
                    double nz = 0.0;
                    for (int e = 0; e < 12; ++e)
                        nz += b_entry(r, e) * s_qp[e] * b_entry(c, e);
#if EQF_BATCH_NORMAL
                    nz += batch_normal_noise_at(pe, r, c);
#else
                    if (r == c)
                        nz += s_qp[12 + (r < 21 ? r / 3 : 7)];
#endif
                    v += dt * nz;
                    S1[r + (size_t)c * ld] = v;
                    S1[c + (size_t)r * ld] = v;
                }
                if (first) { // the gathered rows' readers are behind the barrier above; the next reader is behind the sample's last one
                    for (int r = tid; r < n1; r += BATCH_T)
                        s_gidx[r] = r;
                    first = false;
                }
            }
        }
        // ---- this sample's observer step of the landmarks
        if (wave == 3 && lane < Ns) {
            observer_chain(da.steps + in.obs_off + s, 1, p0, q, a);
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
    if (samples > 0 && !first) { // back into Normal coordinates (the loop's last barrier is behind the last sample's stores)
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
        da.out[blockIdx.x].ric_samples = samples;
        da.out[blockIdx.x].ric_squarings = 0;
    }
