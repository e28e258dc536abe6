// solver_pin.hpp — part of `template <class T> struct Solver` (solver.hip includes this file INSIDE the struct body, after
// solver_path.hpp).  Contents: the pin solve, solver_gaussian_pin_naive.hpp:217-401 / solver_gaussian_pin_cov.hpp:530-705 —
// block coordinate descent along a given lambda path on a screen set that never changes: no screening, no KKT sweep, no
// lambda_max search.  build() has set the state up as for a warm-started Gaussian solve; then, per lambda: fit, record.
//
// The screen set is fixed, so every lambda would pick the same engine.  That decides the route once:
//   * block / panel engines (what pin_solve hands to run_block_passes / run_panel_passes and their group forms): the existing
//     per-lambda fit, rows recorded by update_solutions, exit rules on the host (route 3 / 4);
//   * everything launch_cd takes: the whole path in ONE launch (launch_cd_pin, route 1), or -- config pin_path_launch off --
//     launch_cd once per lambda with a host hand-off in between (route 2).  Both leave the same snapshot block and share
//     everything after it (pin_finish), and they give the same bits: the gradient of the screen values stays where the
//     kernels keep it from lambda to lambda, and the residual is brought up to date once, from the net change of the path.
    bool pin_mode = false;          // set by run_pin before build(): the state checks of a pin state, not of a grpnet state
    const T* pin_sg = nullptr;      // covariance method: the caller's screen_grad (nv values), set before build()
    int pin_path_launch = 1;        // adelie_hip_set_config("pin_path_launch", 0/1) at the time of the call
    int64_t pin_iters = 0, n_pin_launches = 0;
    int pin_route = 0;
    std::vector<T> pin_rsqs, pin_screen_grad;
    std::vector<double> pin_bench_active;
    std::vector<idx> pin_abegins, pin_aorder; // active_begins / active_order of the reference's pin states
    DevBuf<T> d_pin_snap, d_pin_snapg, d_pin_lm, d_pin_g0;
    DevBuf<CdPinRow<T>> d_pin_rows;
    DevBuf<CdPinOut> d_pin_out;

    CdParams<T> pin_cd_params() { // what pin_solve hands the single-workgroup kernels
        CdParams<T> cp{};
        cp.nv = int32_t(nv);
        cp.ns = int32_t(screen_set.size());
        cp.sbegin = d_sbegin.p;
        cp.ssize = d_ssize.p;
        cp.spen = d_spen.p;
        cp.spen2 = nullptr;
        cp.C = d_C.p;
        cp.ldc = ldc;
        cp.vars = d_vars.p;
        cp.xmean = d_sxm.p;
        cp.V = d_V.p;
        cp.voff = d_voff.p;
        cp.beta = d_beta.p;
        cp.g = d_g.p;
        cp.is_active = d_isact.p;
        cp.active_set = d_actset.p;
        cp.lmda = 0;
        cp.alpha = alpha;
        cp.tol = tol; // a pin state's tolerance is absolute (pin_naive:355)
        cp.newton_tol = newton_tol;
        cp.dbeta_tol = T(g_dbeta_tol);
        cp.newton_max_iters = int32_t(std::min<size_t>(newton_max_iters, size_t(1) << 30));
        cp.max_active_size = int32_t(std::min<size_t>(max_active_size, size_t(1) << 30));
        cp.intercept = intercept;
        cp.all_scalar = all_scalar ? 1 : 0;
        cp.max_iters = int64_t(std::min<size_t>(max_iters, size_t(1) << 62));
        cp.sc = d_sc.p;
        cp.beta0 = d_beta0.p;
        cp.vcol = d_vcol.p;
        cp.dcols = d_dcols.p;
        cp.dvals = d_dvals.p;
        cp.max_group_size = int32_t(max_gs);
        return cp;
    }

    static core_error pin_status_error(int status, int l) {
        if (status == CD_MAX_CDS) return max_cds_error(l);
        if (status == CD_MAX_ACTIVE) return make_solver_error("Maximum number of active groups reached.");
        return make_solver_error("Newton-ABS max iterations reached! Try increasing newton_max_iters.");
    }
    bool pin_exit(int l, T rsq_now, T rsq_prev) const {
        return pin_path_exit<T>(cov_mode ? 1 : 0, l, rsq_now, rsq_prev, adev_tol * y_var, ddev_tol * y_var, rdev_tol);
    }

    void solve_pin() {
        if (multi()) throw make_core_error("pin solves are not offered on a multi-response view (kind: multi).");
        if (has_pen2 || cons_on) throw make_core_error("pin solves take neither penalty_l2 nor constraints.");
        const size_t L = lmda_path.size();
        spec_enabled = false;
        inv_wanted = false;
        if (L == 0) return;
        const bool blocks = nv > 0 && !panel_mode() &&
                            ((all_scalar && nv >= cd_block_min_nv) ||
                             (!all_scalar && max_gs <= idx(cd_block_size()) && nv >= cd_block_min_nv));
        if (nv > 0 && (panel_mode() || blocks)) {
            pin_route = panel_mode() ? 4 : 3;
            solve_pin_engines();
            return;
        }
        pin_route = pin_path_launch ? 1 : 2;
        // the gradient of the screen values at the state's coefficients, once
        CdScalars<T> sc{};
        sc.rsq = rsq;
        sc.resid_sum = resid_sum;
        sc.active_size = int32_t(active_set_size);
        d_sc.upload(&sc, 1, st);
        if (nv > 0) {
            if (cov_mode) {
                launch_gather<T>(d_grad.p, d_vcol.p, nv, d_g.p, st); // (build() scattered screen_grad into d_grad)
                d_pin_g0.reserve(size_t(nv));
                AHIP_CHECK(hipMemcpyAsync(d_pin_g0.p, d_g.p, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
            } else {
                cur_w = d_w.p;
                cur_xm = d_xm.p;
                grad_valid = false; // a pin state carries the residual, not the gradient
                load_screen_gradient(d_w.p, d_r.p, &d_sc.p->resid_sum);
            }
            AHIP_CHECK(hipMemcpyAsync(d_beta0.p, d_beta.p, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
        }
        std::vector<CdPinRow<T>> rows(L);
        CdPinOut out{};
        std::vector<double> row_secs(L, 0.0);
        d_pin_snap.reserve(L * size_t(std::max<idx>(nv, 1)));
        if (cov_mode) d_pin_snapg.reserve(L * size_t(std::max<idx>(nv, 1)));
        CdParams<T> cp = pin_cd_params();
        if (nv == 0) {
            // every lambda: one (empty) active pass and one (empty) screen pass with convergence measure 0
            if (!(T(0) < tol)) throw max_cds_error(0);
            CdPinRow<T> r{};
            r.rsq = rsq; r.resid_sum = resid_sum; r.active_size = int32_t(active_set_size);
            T prev = rsq;
            for (size_t l = 0; l < L; ++l) {
                r.iters += 2; r.n_passes_active += 1; r.n_passes_screen += 1;
                rows[l] = r;
                out.n_solved = int32_t(l + 1);
                if (pin_exit(int(l), rsq, prev)) break;
            }
        } else if (pin_route == 1) {
            d_pin_lm.reserve(L);
            d_pin_lm.upload(lmda_path.data(), L, st);
            d_pin_rows.reserve(L);
            d_pin_out.reserve(1);
            CdPinPath<T> pp{};
            pp.lmdas = d_pin_lm.p;
            pp.L = int32_t(L);
            pp.cov = cov_mode ? 1 : 0;
            pp.adev_thr = adev_tol * y_var;
            pp.ddev_thr = ddev_tol * y_var;
            pp.rdev_tol = rdev_tol;
            pp.snap_beta = d_pin_snap.p;
            pp.snap_g = cov_mode ? d_pin_snapg.p : nullptr;
            pp.rows = d_pin_rows.p;
            pp.out = d_pin_out.p;
            t_cd.begin(st);
            launch_cd_pin<T>(cp, pp, st);
            t_cd.end(st);
            ++n_pin_launches;
            d_pin_out.download(&out, 1, st);
            d_pin_rows.download(rows.data(), L, st);
            sync();
            int64_t c0 = out.clock0;
            for (int l = 0; l < out.n_solved; ++l) { // wall_clock64 counts at 100 MHz
                row_secs[size_t(l)] = double(rows[size_t(l)].clock - c0) * 1e-8;
                c0 = rows[size_t(l)].clock;
            }
        } else {
            CdPinRow<T> acc{};
            acc.rsq = rsq; acc.resid_sum = resid_sum; acc.active_size = int32_t(active_set_size);
            T prev = rsq;
            Stopwatch sw;
            for (size_t l = 0; l < L; ++l) {
                sw.start();
                CdScalars<T> s1{};
                s1.rsq = acc.rsq;
                s1.resid_sum = acc.resid_sum;
                s1.active_size = acc.active_size;
                d_sc.upload(&s1, 1, st);
                cp.lmda = lmda_path[l];
                cp.max_iters = int64_t(std::min<size_t>(max_iters, size_t(1) << 62)) - acc.iters; // (the one bound of the path)
                t_cd.begin(st);
                launch_cd<T>(cp, st);
                t_cd.end(st);
                ++n_pin_launches;
                d_sc.download(&s1, 1, st);
                sync();
                if (s1.status != CD_OK) {
                    out.status = s1.status;
                    out.fail_idx = int32_t(l);
                    break;
                }
                acc.rsq = s1.rsq; acc.resid_sum = s1.resid_sum; acc.active_size = s1.active_size;
                acc.iters += s1.iters;
                acc.n_visits_screen += s1.n_visits_screen; acc.n_visits_active += s1.n_visits_active;
                acc.n_updates += s1.n_updates;
                acc.n_passes_screen += s1.n_passes_screen; acc.n_passes_active += s1.n_passes_active;
                rows[l] = acc;
                AHIP_CHECK(hipMemcpyAsync(d_pin_snap.p + l * size_t(nv), d_beta.p, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
                if (cov_mode)
                    AHIP_CHECK(hipMemcpyAsync(d_pin_snapg.p + l * size_t(nv), d_g.p, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
                out.n_solved = int32_t(l + 1);
                row_secs[l] = sw.elapsed();
                const bool stop = pin_exit(int(l), acc.rsq, prev);
                prev = acc.rsq;
                if (stop) break;
            }
        }
        pin_finish(rows, out, row_secs);
    }

    // everything after the snapshot block: the state the last solved lambda left, the rows, the residual
    void pin_finish(const std::vector<CdPinRow<T>>& rows, const CdPinOut& out, const std::vector<double>& row_secs) {
        const size_t n_solved = size_t(out.n_solved);
        const CdPinRow<T>* last = n_solved ? &rows[n_solved - 1] : nullptr;
        const size_t asz = last ? size_t(last->active_size) : active_set_size;
        if (out.status != CD_OK && nv > 0) { // the lambda that failed leaves nothing behind (solver_gaussian_naive.hpp:286-290)
            const T* b_src = last ? d_pin_snap.p + (n_solved - 1) * size_t(nv) : d_beta0.p;
            AHIP_CHECK(hipMemcpyAsync(d_beta.p, b_src, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
            if (cov_mode) {
                const T* g_src = last ? d_pin_snapg.p + (n_solved - 1) * size_t(nv) : d_pin_g0.p;
                AHIP_CHECK(hipMemcpyAsync(d_g.p, g_src, size_t(nv) * sizeof(T), hipMemcpyDeviceToDevice, st));
            }
        }
        std::vector<int32_t> act(asz);
        if (asz) d_actset.download(act.data(), asz, st);
        std::vector<T> snap(n_solved * size_t(nv));
        if (!snap.empty()) d_pin_snap.download(snap.data(), snap.size(), st);
        if (nv > 0) d_beta.download(screen_beta.data(), size_t(nv), st);
        if (cov_mode) {
            pin_screen_grad.assign(size_t(nv), T(0));
            if (nv > 0) d_g.download(pin_screen_grad.data(), size_t(nv), st);
        } else if (nv > 0) { // r -= X_S (beta - beta at entry), once for the whole path
            launch_cd_compact<T>(d_beta.p, d_beta0.p, d_vcol.p, int(nv), d_dcols.p, d_dvals.p, &d_sc.p->n_delta, st);
            t_axpy.begin(st);
            axpy_cols(d_dcols.p, d_dvals.p, &d_sc.p->n_delta, 0, T(-1), d_r.p);
            t_axpy.end(st);
        }
        sync();
        grad_valid = false;
        for (size_t i = 0; i < asz; ++i) active_set[i] = act[i];
        active_set_size = asz;
        std::fill(screen_is_active.begin(), screen_is_active.end(), int8_t(0));
        for (size_t i = 0; i < asz; ++i) screen_is_active[size_t(act[i])] = 1;
        if (out.status != CD_OK && !screen_is_active.empty()) {
            d_isact.upload(screen_is_active.data(), screen_is_active.size(), st);
            sync();
        }
        if (last) {
            rsq = last->rsq;
            resid_sum = last->resid_sum;
            pin_iters = last->iters;
            cnt.n_cd_visits_screen += last->n_visits_screen;
            cnt.n_cd_visits_active += last->n_visits_active;
            cnt.n_updates += last->n_updates;
            cnt.n_cd_passes_screen += last->n_passes_screen;
            cnt.n_cd_passes_active += last->n_passes_active;
        }
        // rows (pin_rows_host.hpp)
        const std::vector<int64_t> sset(screen_set.begin(), screen_set.end()), sbeg(screen_begins.begin(), screen_begins.end());
        const std::vector<int64_t> aset(active_set.begin(), active_set.begin() + asz);
        PinLayout lay{sset.data(), sbeg.data(), groups.data(), group_sizes.data(), int64_t(sset.size()), int64_t(nv), int64_t(G)};
        std::vector<int32_t> row_active(n_solved);
        for (size_t l = 0; l < n_solved; ++l) row_active[l] = rows[l].active_size;
        pin_assemble_rows<T>(lay, snap.data(), row_active.data(), int64_t(n_solved), aset.data(), int64_t(asz), betas_idx, betas_val);
        int64_t vs0 = 0, va0 = 0;
        for (size_t l = 0; l < n_solved; ++l) {
            intercepts.push_back(T(intercept) * (y_mean + rows[l].resid_sum));
            lmdas.push_back(lmda_path[l]);
            pin_rsqs.push_back(rows[l].rsq);
            duals_idx.emplace_back();
            duals_val.emplace_back();
            // one kernel interleaves active and screen passes: the lambda's time is split by its visit counts
            const double va = double(rows[l].n_visits_active - va0), vs = double(rows[l].n_visits_screen - vs0);
            va0 = rows[l].n_visits_active;
            vs0 = rows[l].n_visits_screen;
            const double ta = (va + vs) > 0 ? row_secs[l] * va / (va + vs) : 0;
            pin_bench_active.push_back(ta);
            benchmark_screen.push_back(row_secs[l] - ta);
        }
        if (out.status != CD_OK) throw pin_status_error(out.status, out.fail_idx);
    }

    // the block / panel engines: one existing fit per lambda
    void solve_pin_engines() {
        const size_t L = lmda_path.size();
        const size_t max_iters_all = max_iters;
        struct Restore { size_t& m; size_t v; ~Restore() { m = v; } } restore{max_iters, max_iters_all};
        T prev = rsq;
        if (cov_mode) grad_valid = true; // (d_grad holds v - A beta on the screen positions: what cov_fit gathers)
        for (size_t l = 0; l < L; ++l) {
            const T lm = lmda_path[l];
            const int64_t used = cnt.n_cd_passes_screen + cnt.n_cd_passes_active; // one pass, one iteration (pin_naive:327)
            max_iters = size_t(std::max<int64_t>(0, int64_t(std::min<size_t>(max_iters_all, size_t(1) << 62)) - used));
            FitOut<T> fo;
            try {
                if (cov_mode) {
                    fo = cov_fit(lm);
                } else {
                    CdScalars<T> sc{};
                    sc.resid_sum = resid_sum;
                    d_sc.upload(&sc, 1, st);
                    cur_w = d_w.p;
                    cur_xm = d_xm.p;
                    grad_valid = false; // a pin state carries the residual, not the gradient
                    if (!panel_mode()) load_screen_gradient(d_w.p, d_r.p, &d_sc.p->resid_sum);
                    T rsum = resid_sum;
                    fo = pin_solve(lm, tol, rsq, rsum, y_mean, d_r.p);
                    resid_sum = rsum;
                    rsq = fo.rsq;
                }
            } catch (const core_error& e) {
                pin_iters = cnt.n_cd_passes_screen + cnt.n_cd_passes_active;
                if (std::string(e.what()).find("max coordinate descents reached") != std::string::npos) throw max_cds_error(int(l));
                throw;
            }
            n_pin_launches += 1;
            update_solutions(fo, lm);
            pin_rsqs.push_back(fo.rsq);
            benchmark_screen.push_back(fo.t_screen);
            pin_bench_active.push_back(fo.t_active);
            pin_iters = cnt.n_cd_passes_screen + cnt.n_cd_passes_active;
            if (cov_mode) update_invariance(lm); // grad = v - A beta: the next lambda's screen gradient
            const bool stop = pin_exit(int(l), fo.rsq, prev);
            prev = fo.rsq;
            if (stop) break;
        }
    }

    // after finalize(): the derived vectors of a pin state
    void pin_collect() {
        if (cov_mode && pin_route >= 3) { // the engines keep the full gradient; the screen part of it
            pin_screen_grad.assign(size_t(nv), T(0));
            for (idx a = 0; a < nv; ++a) pin_screen_grad[size_t(a)] = grad[size_t(h_vcol[size_t(a)])];
        }
        const std::vector<int64_t> sset(screen_set.begin(), screen_set.end()), sbeg(screen_begins.begin(), screen_begins.end());
        const std::vector<int64_t> aset(active_set.begin(), active_set.begin() + active_set_size);
        PinLayout lay{sset.data(), sbeg.data(), groups.data(), group_sizes.data(), int64_t(sset.size()), int64_t(nv), int64_t(G)};
        pin_abegins = ahip::pin_active_begins(lay, aset.data(), int64_t(aset.size()));
        pin_aorder = ahip::pin_active_order(lay, aset.data(), int64_t(aset.size()));
    }

    // covariance method, after build(): the caller's screen_grad becomes the screen part of d_grad (what the fits gather), and
    // without cov_v the linear term on the screen positions is put back together as v_S = screen_grad + A_SS beta_S
    void pin_cov_setup(bool have_v) {
        if (!cov_mode || nv == 0) return;
        d_g.upload(pin_sg, size_t(nv), st);
        launch_scatter<T>(d_g.p, d_vcol.p, nv, d_grad.p, st);
        sync();
        if (have_v) return;
        std::vector<T> v(size_t(p), T(0));
        bool warm = false;
        for (idx a = 0; a < nv; ++a) warm = warm || screen_beta[size_t(a)] != T(0);
        std::vector<T> C;
        if (warm) { // d_C holds A_SS (update_gram_and_vars gathered it)
            C.resize(size_t(nv) * size_t(nv));
            AHIP_CHECK(hipMemcpy2DAsync(C.data(), size_t(nv) * sizeof(T), d_C.p, size_t(ldc) * sizeof(T), size_t(nv) * sizeof(T),
                                        size_t(nv), hipMemcpyDeviceToHost, st));
            sync();
        }
        for (idx a = 0; a < nv; ++a) {
            T acc = pin_sg[a];
            if (warm)
                for (idx b = 0; b < nv; ++b) acc += C[size_t(a) + size_t(b) * size_t(nv)] * screen_beta[size_t(b)];
            v[size_t(h_vcol[size_t(a)])] = acc;
        }
        d_covv.upload(v.data(), size_t(p), st);
        sync();
    }
