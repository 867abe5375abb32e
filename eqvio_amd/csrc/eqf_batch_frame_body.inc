// The body of k_batch_frame (eqf_batch.hpp), included once per kernel: with EQF_BATCH_FRAME_TAIL 0 the whole frame (k_batch_frame: the text the kernel has
// always had, so that it compiles to the code it has always had - as a function template shared with the tail the same statements came out of the register
// allocator 17 % slower, 768 against 656 us at B = 256), with EQF_BATCH_FRAME_TAIL 1 phases 2 - 5 alone (k_batch_frame_tail), behind k_batch_riccati, which
// leaves what phases 0 and 1 leave: the propagated Sigma of the surviving landmarks in the slot's other Sigma buffer, their planes in the other landmark buffer.
// `ba` is the kernel's BatchArgs.
    __shared__ double sm[BATCH_SM];
    __shared__ int s_gidx[BATCH_NMAX];
    __shared__ int s_surv[BATCH_L], s_keep[BATCH_L], s_mlm[BATCH_L], s_mj[BATCH_L];
    __shared__ int s_misc[8]; // 0 kept, 1 matched, 2 fail, 3 kept after the lift
    __shared__ double s_depth;
    __shared__ unsigned long long s_mask;
    const BatchIn& in = ba.in[blockIdx.x];
    BatchOut* out = ba.out + blockIdx.x;
    const int tid = threadIdx.x;
    const int L = BATCH_L, ld = ba.buf.ld;
    // the slot's settings: read once, before the first store of the launch
    const int chart = in.ss.chart, star = in.ss.star, discrete = in.ss.discrete, median = in.ss.median;
    const double thrAbs = in.ss.thrAbs, thrProb = in.ss.thrProb, meas_var = in.ss.meas_var, init_var = in.ss.init_var, init_depth = in.ss.init_depth;
    const bool ind = chart == EQVIO_COORD_INVDEPTH;
    const int slot = in.slot, cur = in.cur, nxt = cur ^ 1;
    double* S0 = ba.buf.sig_of(slot, cur);
    double* S1 = ba.buf.sig_of(slot, nxt);
    double* L0 = ba.buf.lm_of(slot, cur);
    double* L1 = ba.buf.lm_of(slot, nxt);
    double* scr = ba.buf.scr_of(slot);
    const int Ns = in.Ns, n1 = 21 + 3 * Ns, M = in.M;
#if !EQF_BATCH_FRAME_TAIL
    const double dt = in.dt;

    // ---- phase 0: A / B rows, landmark planes, observer steps
    double* Ass = sm;
    double* Bs = sm + 441;
    double* lm66 = sm + 693;
    double* Al = sm + 759;
    double* Bl = Al + BATCH_L * 45;
    double* Qd = sm + BATCH_SM_PROP; // the slot's input gains and process variances, behind the rows (the update's region is the larger one)
    double* Pd = Qd + 12;
    if (tid < 12)
        Qd[tid] = in.ss.Qd[tid];
    else if (tid < 20)
        Pd[tid - 12] = in.ss.Pd[tid - 12];
    for (int t = tid; t < 441; t += BATCH_T)
        Ass[t] = sensor_Ass_entry(in.ck, t);
    for (int t = tid; t < 252; t += BATCH_T)
        Bs[t] = sensor_Bs_entry(in.ck, t);
    for (int t = tid; t < 66; t += BATCH_T)
        lm66[t] = in.ck.lm[t];
    for (int t = tid; t < Ns; t += BATCH_T)
        s_surv[t] = in.surv[t];
    __syncthreads();
    for (int r = tid; r < n1; r += BATCH_T)
        s_gidx[r] = r < 21 ? r : 21 + 3 * s_surv[(r - 21) / 3] + (r - 21) % 3;
    {
        // waves 0 / 1 / 2 assemble the three independent column parts of a landmark's rows of A and B (assemble_landmark<PART>), wave 3 copies its planes and
        // runs the observer steps: one lane per landmark in each
        const int wave = tid >> 6, i = tid & 63;
        if (i < Ns) {
            const int o = s_surv[i];
            const V3 p0 = ld3(L0, L, o);
            Qt q = ldq(L0 + BATCH_QQ * L, L, o);
            double a = L0[BATCH_QA * L + o];
            if (wave < 3) {
                const M3 e2i = ind ? ld_cc(L0, L, o, CC_E2I) : M3{}, i2e = ind && wave == 2 ? ld_cc(L0, L, o, CC_I2E) : M3{};
                double al[45], bl[9];
                if (wave == 0) {
                    assemble_landmark<0>(lm66, chart, p0, q, a, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 6; ++c)
                            Al[i * 45 + r * 15 + c] = al[r * 15 + c];
                    for (int e = 0; e < 9; ++e)
                        Bl[i * 9 + e] = bl[e];
                } else if (wave == 1) {
                    assemble_landmark<1>(lm66, chart, p0, q, a, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 6; c < 12; ++c)
                            Al[i * 45 + r * 15 + c] = al[r * 15 + c];
                } else {
                    assemble_landmark<2>(lm66, chart, p0, q, a, e2i, i2e, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 12; c < 15; ++c)
                            Al[i * 45 + r * 15 + c] = al[r * 15 + c];
                }
            } else {
                for (int pl = 0; pl < BATCH_QQ; ++pl)
                    L1[pl * L + i] = L0[pl * L + o];
                if (in.k > 0)
                    observer_chain(ba.steps + in.obs_off, in.k, p0, q, a);
                L1[BATCH_QQ * L + i] = q.w;
                L1[(BATCH_QQ + 1) * L + i] = q.x;
                L1[(BATCH_QQ + 2) * L + i] = q.y;
                L1[(BATCH_QQ + 3) * L + i] = q.z;
                L1[BATCH_QA * L + i] = a;
            }
        }
    }
    __syncthreads();

    // row r of F = I + dt A applied to a vector given entry by entry: sum_k F[r][k] v(k)
    auto f_row = [&](int r, auto v) -> double {
        double acc = 0.0;
        if (r < 21) {
            for (int k = 0; k < 21; ++k)
                acc += Ass[r * 21 + k] * v(k);
        } else {
            const int i = (r - 21) / 3, a = (r - 21) % 3;
            const double* row = Al + i * 45 + a * 15;
            for (int e = 0; e < 12; ++e)
                acc += row[e] * v(al_col(e));
            for (int b = 0; b < 3; ++b)
                acc += row[12 + b] * v(21 + 3 * i + b);
        }
        return v(r) + dt * acc;
    };
    auto b_entry = [&](int r, int e) -> double {
        if (r < 21)
            return Bs[r * 12 + e];
        const int i = (r - 21) / 3, a = (r - 21) % 3;
        return e < 3 ? Bl[i * 9 + a * 3 + e] : 0.0;
    };

    // ---- phase 1: Sigma' = F Sigma F^T + dt (B Q B^T + P)
    double* G = scr;
    for (int t = tid; t < n1 * n1; t += BATCH_T) {
        const int r = t % n1, c = t / n1;
        const double* col = S0 + (size_t)s_gidx[c] * ld;
        G[r + (size_t)c * ld] = f_row(r, [&](int k) { return col[s_gidx[k]]; });
    }
    __syncthreads();
    for (int t = tid; t < n1 * n1; t += BATCH_T) {
        const int r = t % n1, c = t / n1;
        if (r < c)
            continue;
        double v = f_row(c, [&](int k) { return G[r + (size_t)k * ld]; });
        double nz = 0.0;
        for (int e = 0; e < 12; ++e)
            nz += b_entry(r, e) * Qd[e] * b_entry(c, e);
        if (r == c)
            nz += Pd[r < 21 ? r / 3 : 7];
        v += dt * nz;
        S1[r + (size_t)c * ld] = v;
        S1[c + (size_t)r * ld] = v;
    }
    __syncthreads();
#endif

    // ---- phase 2: removeOutliers
    double* ylm = scr + (size_t)ld * BATCH_NMAX; // planes u, v, feature index (-1: not measured)
    double* stats = ylm + 3 * L;                 // absErr, probErr, |q_hat|^2 of the surviving landmarks
    for (int i = tid; i < Ns; i += BATCH_T)
        ylm[2 * L + i] = -1.0;
    __syncthreads();
    for (int j = tid; j < M; j += BATCH_T)
        if (in.midx[j] >= 0) {
            const int i = in.midx[j];
            ylm[i] = in.y[2 * j];
            ylm[L + i] = in.y[2 * j + 1];
            ylm[2 * L + i] = (double)j;
        }
    __syncthreads();
    if (tid < Ns) {
        double ae, pe;
        outlier_stats_body<double>(Ns, L, ld, chart, in.cam, ylm, L1, L1 + BATCH_QQ * L, L1 + BATCH_QA * L, S1, stats, 0, nullptr, nullptr, nullptr, nullptr, ae, pe,
                                   false, tid);
    }
    __syncthreads();
    if (tid == 0) {
        // candidates ranked as the reference's sort + reverse: absolute outliers first (largest error first), then probabilistic ones
        unsigned long long cand = 0, drop = 0;
        for (int i = 0; i < Ns; ++i) {
            const double ae = stats[i], pe = stats[Ns + i];
            if (ylm[2 * L + i] < 0.0)
                continue;
            if (ae > thrAbs || pe > thrProb)
                cand |= 1ull << i;
        }
        for (int t = 0; t < in.max_outliers && cand; ++t) {
            int best = -1;
            bool best_abs = false;
            double best_v = 0.0;
            for (int i = 0; i < Ns; ++i) {
                if (!((cand >> i) & 1ull))
                    continue;
                const bool isabs = stats[i] > thrAbs;
                const double v = isabs ? stats[i] : stats[Ns + i];
                if (best < 0 || (isabs && !best_abs) || (isabs == best_abs && v > best_v)) {
                    best = i;
                    best_abs = isabs;
                    best_v = v;
                }
            }
            cand &= ~(1ull << best);
            drop |= 1ull << best;
        }
        int nk = 0;
        for (int i = 0; i < Ns; ++i)
            if (!((drop >> i) & 1ull))
                s_keep[nk++] = i;
        // getMedianSceneDepth over the landmarks that stay: the element nth_element puts at position nk / 2
        double depth = init_depth;
        if (median && nk > 0) {
            const int kth = nk / 2;
            for (int a = 0; a < nk; ++a) {
                const double va = stats[2 * Ns + s_keep[a]];
                int less = 0, eq = 0;
                for (int b = 0; b < nk; ++b) {
                    const double vb = stats[2 * Ns + s_keep[b]];
                    less += vb < va;
                    eq += vb == va;
                }
                if (less <= kth && kth < less + eq) {
                    depth = sqrt(va);
                    break;
                }
            }
        }
        // the matched measurement: features of kept or new landmarks, ascending id; their landmark index after addNewLandmarks
        int m2 = 0;
        for (int j = 0; j < M; ++j) {
            const int mi = in.midx[j];
            int li;
            if (mi >= 0) {
                if ((drop >> mi) & 1ull)
                    continue;
                li = 0;
                for (int a = 0; a < mi; ++a)
                    li += !((drop >> a) & 1ull);
            } else {
                li = nk + (-mi - 1);
            }
            s_mlm[m2] = li;
            s_mj[m2] = j;
            ++m2;
        }
        s_misc[0] = nk;
        s_misc[1] = m2;
        s_misc[2] = 0;
        s_depth = depth;
        out->outliers = drop;
        out->depth = depth;
        out->did = (drop ? BATCH_DID_OUTLIERS : 0) | (in.nnew ? BATCH_DID_ADDED : 0);
    }
    __syncthreads();

    // ---- phase 3: the kept landmarks and the new ones back to the first buffer pair
    const int nk = s_misc[0], N2 = nk + in.nnew, n2 = 21 + 3 * N2, M2 = s_misc[1];
    for (int r = tid; r < n2; r += BATCH_T)
        s_gidx[r] = r < 21 ? r : ((r - 21) / 3 < nk ? 21 + 3 * s_keep[(r - 21) / 3] + (r - 21) % 3 : -1);
    __syncthreads();
    batch_gather_sigma(S0, S1, s_gidx, n2, ld, init_var);
    if (tid < N2) {
        const int i = tid;
        if (i < nk) {
            for (int pl = 0; pl < BATCH_PLANES; ++pl)
                L0[pl * L + i] = L1[pl * L + s_keep[i]];
        } else {
            const int r = i - nk;
            const double d = s_depth;
            batch_new_landmark(L0, i, in.bear[3 * r] * d, in.bear[3 * r + 1] * d, in.bear[3 * r + 2] * d);
        }
    }
    __syncthreads();
    if (M2 == 0) { // performVisionUpdate returns at once on an empty measurement, and processVisionData before removeInvalidLandmarks
        if (tid == 0) {
            out->did |= BATCH_DID_EMPTY;
            batch_finish(out, 0, N2, cur, 0, 0, 0.0, 0.0);
        }
        return;
    }

    // ---- phase 4: performVisionUpdate
    const int m = 2 * M2;
    double* Sp = sm;                  // S, then L: packed lower triangle
    double* Cb = Sp + BATCH_SPACK;    // output blocks, 6 per matched feature
    double* yt = Cb + BATCH_L * 6;    // yTilde
    double* z = yt + BATCH_MAXM;      // L^-1 yTilde
    double* gam = z + BATCH_MAXM;     // Gamma
    double* inn = gam + BATCH_NMAX;   // NIS, log det S (the region's last three doubles are not Gamma's)
    if (tid < M2) {
        const int i = s_mlm[tid], j = s_mj[tid];
        const MeasOut o = measure_one(chart, in.cam, ld3(L0, L, i), ldq(L0 + BATCH_QQ * L, L, i), L0[BATCH_QA * L + i], in.y[2 * j], in.y[2 * j + 1], star != 0,
                                      ind ? ld_cc(L0, L, i, CC_R0) : M3{});
        for (int e = 0; e < 6; ++e)
            Cb[tid * 6 + e] = o.c[e];
        yt[2 * tid] = o.yt[0];
        yt[2 * tid + 1] = o.yt[1];
    }
    __syncthreads();
    double* T = scr; // T = Sigma C^T (n2 x m), then W^T in place
    for (int t = tid; t < n2 * M2; t += BATCH_T) {
        const int r = t % n2, jj = t / n2;
        const int l = 21 + 3 * s_mlm[jj];
        double cj[6];
        for (int e = 0; e < 6; ++e)
            cj[e] = Cb[jj * 6 + e];
        double o0, o1;
        bz_T_pair(S0[r + (size_t)l * ld], S0[r + (size_t)(l + 1) * ld], S0[r + (size_t)(l + 2) * ld], cj, o0, o1);
        T[r + (size_t)(2 * jj) * ld] = o0;
        T[r + (size_t)(2 * jj + 1) * ld] = o1;
    }
    for (int t = tid; t < M2 * M2; t += BATCH_T) {
        const int ii = t % M2, jj = t / M2;
        if (ii < jj)
            continue;
        const int li = 21 + 3 * s_mlm[ii], lj = 21 + 3 * s_mlm[jj];
        double ci[6], cj[6], sv[9], o[2][2];
        for (int e = 0; e < 6; ++e) {
            ci[e] = Cb[ii * 6 + e];
            cj[e] = Cb[jj * 6 + e];
        }
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r)
                sv[3 * c + r] = S0[(li + r) + (size_t)(lj + c) * ld];
        bz_S_block(ci, cj, sv, ii == jj, meas_var, o);
        Sp[bt_tri(2 * ii, 2 * jj)] = o[0][0];
        Sp[bt_tri(2 * ii + 1, 2 * jj)] = o[1][0];
        Sp[bt_tri(2 * ii + 1, 2 * jj + 1)] = o[1][1];
        if (ii != jj)
            Sp[bt_tri(2 * ii, 2 * jj + 1)] = o[0][1];
    }
    __syncthreads();
    // Cholesky S = L L^T, right-looking, in LDS
    for (int k = 0; k < m; ++k) {
        if (tid == 0) {
            const double d = Sp[bt_tri(k, k)];
            if (!(d > 0.0) || !(d - d == 0.0))
                s_misc[2] = 1;
            Sp[bt_tri(k, k)] = sqrt(d);
        }
        __syncthreads();
        if (s_misc[2])
            break;
        const double lkk = Sp[bt_tri(k, k)];
        for (int i = k + 1 + tid; i < m; i += BATCH_T)
            Sp[bt_tri(i, k)] = Sp[bt_tri(i, k)] / lkk;
        __syncthreads();
        for (int i = k + 1 + tid; i < m; i += BATCH_T) {
            const double lik = Sp[bt_tri(i, k)];
            for (int j = k + 1; j <= i; ++j)
                Sp[bt_tri(i, j)] -= lik * Sp[bt_tri(j, k)];
        }
        __syncthreads();
    }
    if (s_misc[2]) {
        if (tid == 0)
            batch_finish(out, EQF_E_NOT_SPD, N2, cur, 0, m, __builtin_nan(""), __builtin_nan(""));
        return;
    }
    // W^T = T L^-T and z^T = yTilde^T L^-T, blocked by 16 columns on the matrix cores: row tiles of 16 rows of [T ; yTilde^T] (one wave each); per column block
    // kb the product with the finished blocks (mfma16_nt, v_mfma_f64_16x16x4_f64) and then the 16 x 16 triangle, one lane per row. The columns are padded to
    // m16 (zero columns of T, identity rows of L): the padding stays zero.
    const int m16 = (m + 15) & ~15, rows = n2 + 1, nrt = (rows + 15) / 16;
    double* Ld = scr + (size_t)ld * BATCH_MAXM; // L dense, column stride BATCH_MAXM
    for (int t = tid; t < m16 * m16; t += BATCH_T) {
        const int i = t % m16, p = t / m16;
        Ld[i + (size_t)p * BATCH_MAXM] = (i < m && p < m) ? (p <= i ? Sp[bt_tri(i, p)] : 0.0) : (i == p ? 1.0 : 0.0);
    }
    for (int t = tid; t < nrt * 16 * m16; t += BATCH_T) {
        const int r = t % (nrt * 16), k = t / (nrt * 16);
        if (r == n2)
            T[r + (size_t)k * ld] = k < m ? yt[k] : 0.0;
        else if (r > n2 || k >= m)
            T[r + (size_t)k * ld] = 0.0;
    }
    __syncthreads();
    {
        const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
        for (int rt = wave; rt < nrt; rt += BATCH_T / 64) {
            double* Tr = T + rt * 16;
            for (int kb = 0; kb < m16 / 16; ++kb) {
                d4 acc = {0, 0, 0, 0};
                for (int pb = 0; pb < kb; ++pb) {
                    const d4 a = mfma16_nt(Tr + (size_t)pb * 16 * ld, ld, Ld + kb * 16 + (size_t)pb * 16 * BATCH_MAXM, BATCH_MAXM);
                    acc[0] += a[0], acc[1] += a[1], acc[2] += a[2], acc[3] += a[3];
                }
                for (int q = 0; q < 4; ++q) {
                    double* e = Tr + lr + (size_t)(kb * 16 + lk + 4 * q) * ld;
                    *e -= acc[q];
                }
                batch_wave_sync();
                if (lane < 16) { // the diagonal block: row lr of the tile against L[kb block][kb block]
                    double x[16];
                    for (int c = 0; c < 16; ++c) {
                        const double* lc = Ld + kb * 16 + c; // L[kb * 16 + c][kb * 16 + p] at lc[(kb * 16 + p) * BATCH_MAXM]
                        double v = Tr[lane + (size_t)(kb * 16 + c) * ld];
                        for (int p = 0; p < c; ++p)
                            v -= lc[(size_t)(kb * 16 + p) * BATCH_MAXM] * x[p];
                        x[c] = v / lc[(size_t)(kb * 16 + c) * BATCH_MAXM];
                        Tr[lane + (size_t)(kb * 16 + c) * ld] = x[c];
                    }
                }
                batch_wave_sync();
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < m; k += BATCH_T)
        z[k] = T[n2 + (size_t)k * ld];
    __syncthreads();
    for (int t = tid; t < n2; t += BATCH_T) {
        double g = 0.0;
        for (int k = 0; k < m; ++k)
            g += T[t + (size_t)k * ld] * z[k];
        gam[t] = g;
        if (!(g - g == 0.0))
            s_misc[2] = 2;
    }
    // The innovation statistics, from what the solve left in LDS: NIS = |z|^2 (wave 0) and log det S = 2 sum log L_kk (wave 1), over the true m rows. Lane l
    // adds its entries l, l + 64 in ascending order, then the wave's butterfly: the order depends on m alone, not on the workgroup or the step's slot count.
    if (tid < 128) {
        const int lane = tid & 63;
        double v = 0.0;
        if (tid < 64) {
            for (int k = lane; k < m; k += 64)
                v += z[k] * z[k];
        } else {
            for (int k = lane; k < m; k += 64)
                v += log(Sp[bt_tri(k, k)]);
        }
        v = batch_wave_sum(v);
        if (lane == 0)
            inn[tid >> 6] = tid < 64 ? v : 2.0 * v;
    }
    __syncthreads();
    if (s_misc[2]) {
        if (tid == 0)
            batch_finish(out, EQF_E_NONFINITE, N2, cur, 0, m, __builtin_nan(""), __builtin_nan(""));
        return;
    }
    // Sigma -= W^T W on the matrix cores: lower 16 x 16 tiles (one wave each), K = m16 (the padded columns of W are zero), mirrored into the upper half
    {
        const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
        const int nt = (n2 + 15) / 16;
        for (int t = wave; t < nt * (nt + 1) / 2; t += BATCH_T / 64) {
            int bi, bj;
            batch_tri_tile(t, bi, bj);
            d4 acc = {0, 0, 0, 0};
            for (int pb = 0; pb < m16 / 16; ++pb) {
                const d4 a = mfma16_nt(T + bi * 16 + (size_t)pb * 16 * ld, ld, T + bj * 16 + (size_t)pb * 16 * ld, ld);
                acc[0] += a[0], acc[1] += a[1], acc[2] += a[2], acc[3] += a[3];
            }
            const int r = bi * 16 + lr;
            for (int q = 0; q < 4; ++q) {
                const int c = bj * 16 + lk + 4 * q;
                if (r < n2 && c < n2 && (bi > bj || r >= c)) {
                    const double v = S0[r + (size_t)c * ld] - acc[q];
                    S0[r + (size_t)c * ld] = v;
                    S0[c + (size_t)r * ld] = v;
                }
            }
        }
    }
    // landmark lift; the sensor rows go to the host
    double* est = ylm; // 4 planes of stride N2 (estimate, invalid flag)
    if (tid < N2) {
        const int i = tid;
        const LiftIn li = lift_load(i, L, chart, discrete, L0, L0 + BATCH_QQ * L, L0 + BATCH_QA * L);
        lift_landmark(i, V3{gam[21 + 3 * i], gam[22 + 3 * i], gam[23 + 3 * i]}, li, N2, L, chart, discrete, L0 + BATCH_QQ * L, L0 + BATCH_QA * L, est);
    }
    if (tid < 21)
        out->gamma[tid] = gam[tid];
    __syncthreads();

    // ---- phase 5: removeInvalidLandmarks
    if (tid == 0) {
        unsigned long long bad = 0;
        int nk2 = 0;
        for (int i = 0; i < N2; ++i) {
            if (est[3 * N2 + i] != 0.0)
                bad |= 1ull << i;
            else
                s_keep[nk2++] = i;
        }
        s_misc[3] = nk2;
        s_mask = bad;
    }
    __syncthreads();
    const int N3 = s_misc[3];
    if (N3 < N2) {
        const int n3 = 21 + 3 * N3;
        for (int r = tid; r < n3; r += BATCH_T)
            s_gidx[r] = r < 21 ? r : 21 + 3 * s_keep[(r - 21) / 3] + (r - 21) % 3;
        __syncthreads();
        for (int t = tid; t < n3 * n3; t += BATCH_T) {
            const int r = t % n3, c = t / n3;
            S1[r + (size_t)c * ld] = S0[s_gidx[r] + (size_t)s_gidx[c] * ld];
        }
        if (tid < N3)
            for (int pl = 0; pl < BATCH_PLANES; ++pl)
                L1[pl * L + tid] = L0[pl * L + s_keep[tid]];
    }
    if (tid == 0) {
        out->did |= BATCH_DID_UPDATE | (N3 < N2 ? BATCH_DID_INVALID : 0);
        batch_finish(out, 0, N3, N3 < N2 ? nxt : cur, s_mask, m, inn[0], inn[1]);
    }
