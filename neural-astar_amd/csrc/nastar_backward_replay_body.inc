// nastar_backward_replay_body.inc -- the body of nastar_backward_replay_kernel and nastar_backward_replay_masked_kernel
// (nastar_backward_replay.hip.h), included INSIDE each kernel so that the kernel without a mask keeps its instruction stream (see
// nastar_forward_compact_body.inc).  In scope: kGlobal, kHistLds, kFastDiv, kWide, `a`, `rcp_sqrtW`, and `constexpr bool kMasked` / `nmask`, `constexpr bool kHeur` / `h0p`,
// and `constexpr bool kMulti` (nastar_backward_replay_sources_kernel, include/nastar_sources.h): every non-zero cell of the start map is open from
// history index 0, so the initial softmax sums run over all of them.
    static_assert(!kWide || kGlobal, "wide stamps exist for the HBM state only");
    using stamp_t = typename std::conditional<kWide, uint32_t, unsigned short>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = (a.order == nullptr || (a.order_bad != nullptr && *a.order_bad != 0)) ? (int)blockIdx.x : a.order[blockIdx.x];
    if ((unsigned)b >= (unsigned)a.B_total) return;  // not a permutation: never touch memory outside the batch
    const int lane = threadIdx.x;
    const CompactDims d = a.d;
    unsigned char* base = kGlobal ? a.state + (size_t)b * a.state_stride : smem;
    float* g = reinterpret_cast<float*>(base);                 // [HWp] g-value / node state (sign of infinity, as the forward)
    float* cst = g + d.HWp;                                     // [HWp] cost
    float* G = cst + d.HWp;                                     // [HWp] upstream gradient
    stamp_t* t0 = reinterpret_cast<stamp_t*>(G + d.HWp);  // [HWp] history index at which the cell was (re)opened
    double* sd = reinterpret_cast<double*>(smem + (kGlobal ? 0 : (size_t)d.HWp * 14));  // S, D: always in LDS
    const size_t off = (size_t)b * (size_t)d.HW;
    // h0 of cell `i` at (r, c): the built-in heuristic from the coordinates, or (kHeur: nastar_backward_replay_heuristic_kernel, `h0p` = the
    // caller's heuristic maps) the value the forward searched with, read from the tensor
    const float* const h0m = kHeur ? h0p + off : nullptr;
    auto h0 = [=](int i, int r, int c, int gr, int gc) {
        if constexpr (kHeur) return h0m[i];
        else return kWide ? heuristic0(r, c, gr, gc) : heuristic0_fast(r, c, gr, gc);
    };
    static_assert(!(kGlobal && kHistLds), "a map too large for LDS keeps its history in the workspace as well");
    double* hist = kHistLds ? reinterpret_cast<double*>(smem + (size_t)d.HWp * 14 + 16) : a.hist + (size_t)b * (size_t)a.hist_len * 2;
    float* gout = a.grad_cost + off;

    int sidx = -1, gidx = -1;
    int* const hdr = kGlobal ? reinterpret_cast<int*>(base + bwdr_header_offset(d.HWp, kWide)) : nullptr;
    if constexpr (kGlobal) {  // the fill launch initialised the slab and found the start / goal cells
        sidx = __builtin_amdgcn_readfirstlane(hdr[0]);
        gidx = __builtin_amdgcn_readfirstlane(hdr[1]);
    } else {
        for (int i = lane; i < d.HW; i += 64) {
            if (a.start[off + i] != 0.f) sidx = i;
            if (a.goal[off + i] != 0.f) gidx = i;
            st_st<kGlobal>(&g[i], a.passable[off + i] != 0.f ? NASTAR_POS_INF : NASTAR_NEG_INF);
            st_st<kGlobal>(&cst[i], a.cost[off + i]);
            st_st<kGlobal>(&G[i], bwdr_upstream(a, off + i));
            st_st<kGlobal>(&t0[i], (stamp_t)0);
            gout[i] = 0.f;
        }
        sidx = wave_max_i32(sidx);
        gidx = wave_max_i32(gidx);
    }
    if (lane == 0) {
        sd[0] = 0.0;
        sd[1] = 0.0;
        hist_st<kHistLds>(&hist[0], 0.0);
        hist_st<kHistLds>(&hist[1], 0.0);
    }
    global_step_fence();  // the zeroed gradient and history entry 0 are in L2 before any atomic / load touches them
    wave_sync();
    if (sidx < 0 || gidx < 0) return;

    const int goal_r = gidx / d.W, goal_c = gidx - goal_r * d.W;
    const int n_steps = a.iters[b];
    // The reference keeps stepping a finished map at its fixed point until the slowest map of the batch is done (:251):
    // extra = t_batch - tau such steps; the goal cell is then re-selected while closed and torch.clamp's backward (:223) zeroes
    // its upstream gradient.
    int extra = 0;
    if (a.t_batch != nullptr) extra = *a.t_batch - (n_steps - 1);
    const int* log = a.sel_log + (size_t)b * (size_t)a.max_iters;
    // A log written in LOCK-STEP mode (nastar_forward_batchloop_finish: a map of the batch-coupled class) may select the goal BEFORE its last
    // entry: the goal is then expanded like any cell and stays open (:224), and every RE-selection finds it in histories already -- clamp's
    // backward (:223) zeroes the goal's upstream gradient for that step and all earlier ones.  An ordinary log selects the goal once, last.
    int n_goal = 0, t_last_goal = -1;
    for (int t = lane; t < n_steps; t += 64)
        if (log[t] == gidx) {
            ++n_goal;
            t_last_goal = t;
        }
    n_goal = (int)wave_sum_f32((float)n_goal);  // (exact: < 2^24 selections)
    t_last_goal = wave_max_i32(t_last_goal);
    const bool goal_zeroed = n_goal + (extra > 0 ? extra : 0) >= 2;
    // ... and from the step after its last re-selection on (budget-truncated runs only) the goal's gradient counts again
    const int t_restore = (goal_zeroed && extra <= 0 && t_last_goal < n_steps - 1) ? t_last_goal : -1;
    const float goal_up = bwdr_upstream(a, off + (size_t)gidx);
    if constexpr (kMulti) {
        if (lane == 0 && goal_zeroed) st_st<kGlobal>(&G[gidx], 0.f);
        // open list = every start cell (:187 open_maps = start_maps), each with g = 0 and open from history index 0: S = sum v, D = sum G v.
        // (fp64 sums of fp32 terms, as every later change of S and D; the goal's zeroed upstream value must be in place first)
        if constexpr (kGlobal) global_step_fence();
        wave_sync();
        double dS = 0.0, dD = 0.0;
        int n_open = 0, last_open = 0;
        auto open = [&](int i) {
            ++n_open;
            last_open = i;
            const int r = i / d.W, c = i - r * d.W;
            const float hh = d.omg * (h0(i, r, c, goal_r, goal_c) + st_ld<kGlobal>(&cst[i]));
            const float v = bwdr_v<kFastDiv>(d, 0.0f, hh, rcp_sqrtW);
            st_st<kGlobal>(&g[i], 0.0f);
            dS += (double)v;
            dD += (double)(st_ld<kGlobal>(&G[i]) * v);
        };
        const float* const sm = a.start + off;
        int done = 0;
        if constexpr (kGlobal) {
            // a large map: ONE wavefront reads the whole start map -- 16 cells per lane and trip, four 16-byte loads in flight (as the
            // forward's seeding pass, hybrid_open_sources), where the map's row is 16-byte aligned
            if ((d.HW & 3) == 0 && (reinterpret_cast<uintptr_t>(sm) & 15u) == 0) {
                const float4* s4 = reinterpret_cast<const float4*>(sm);
                const int n4 = d.HW >> 2;
                int q = lane;
                for (; q + 192 < n4; q += 256) {
                    float4 sv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) sv[k] = s4[q + 64 * k];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = (q + 64 * k) << 2;
                        if (sv[k].x != 0.f) open(i);
                        if (sv[k].y != 0.f) open(i + 1);
                        if (sv[k].z != 0.f) open(i + 2);
                        if (sv[k].w != 0.f) open(i + 3);
                    }
                }
                for (; q < n4; q += 64) {
                    const float4 sv = s4[q];
                    const int i = q << 2;
                    if (sv.x != 0.f) open(i);
                    if (sv.y != 0.f) open(i + 1);
                    if (sv.z != 0.f) open(i + 2);
                    if (sv.w != 0.f) open(i + 3);
                }
                done = d.HW;
            }
        }
        for (int i = done + lane; i < d.HW; i += 64)
            if (sm[i] != 0.f) open(i);
        // ONE source in all: the single-source replay's open list, whose start carries stamp 1 (below) -- the same bits for a one-hot start map
        if ((int)wave_sum_f32((float)n_open) == 1 && n_open == 1) st_st<kGlobal>(&t0[last_open], (stamp_t)1);
        const uint32_t sda0 = (uint32_t)(uintptr_t)sd;
        asm volatile("ds_add_f64 %0, %1\n\tds_add_f64 %0, %2 offset:8" ::"v"(sda0), "v"(dS), "v"(dD) : "memory");
    } else
    if (lane == 0) {
        if (goal_zeroed) st_st<kGlobal>(&G[gidx], 0.f);
        // open list = {start} (:187), g[start] = 0 (:193): the start is open from history index 0
        const int r = sidx / d.W, c = sidx - r * d.W;
        const float hh = d.omg * (h0(sidx, r, c, goal_r, goal_c) + st_ld<kGlobal>(&cst[sidx]));
        const float v = bwdr_v<kFastDiv>(d, 0.0f, hh, rcp_sqrtW);
        st_st<kGlobal>(&g[sidx], 0.0f);
        // ... with stamp 1, not 0: at step 0 the open list is {start}, y = 1 and G - <G, y> is exactly zero (the oracle's reverse mode gives
        // 0.0 there), but kfac v (G rS - (G v) rS rS) in fp32 is not -- 1e-11 .. 1e-8 of noise on the start cell, all there is of a
        // gradient that must be exactly zero (a budget of one step, a start == goal map on its own).  Entry 1 is what step 0 writes.
        st_st<kGlobal>(&t0[sidx], (stamp_t)1);
        sd[0] = (double)v;
        sd[1] = (double)(st_ld<kGlobal>(&G[sidx]) * v);
    }
    if constexpr (kGlobal) global_step_fence();
    wave_sync();

    int dr, dc;
    neighbour_delta(lane & 7, dr, dc);
    const bool is_nb = kMasked ? neighbour_enabled(lane, nmask) : lane < 8;
    const int noff = dr * d.W + dc;
    double A = 0.0, B = 0.0;
    // pending interval (closed in the previous step, its history entry still in flight)
    bool pend = false;
    float pv = 0.f, pG = 0.f;
    int pcell = 0;
    double pA0 = 0.0, pB0 = 0.0, pA = 0.0, pB = 0.0;
    int logv = 0;
    bool goal_fixed_point = false;
    for (int t = 0; t < n_steps; ++t) {
        if ((t & 63) == 0) logv = (t + lane < n_steps) ? log[t + lane] : 0;
        const int s = __builtin_amdgcn_readlane(logv, t & 63);
        // HBM history / state: everything issued so far has landed -- the history entry of the previous step, the loads of the
        // pending intervals, the state stores of the previous step.  (LDS executes a wave's operations in order: nothing to do.)
        if constexpr (kGlobal || !kHistLds) global_step_fence();
        if (pend) {
            const float dA = (float)(pA - pA0), dB = (float)(pB - pB0);
            unsafeAtomicAdd(&gout[pcell], (a.kfac * pv) * (pG * dA - dB));
        }
        // softmax of step t over the current open list: A += 1/S, B += D/S^2   (y_t = v/S, <G,y_t> = D/S)
        const double S = sd[0], D = sd[1];
        const float rS = __builtin_amdgcn_rcpf((float)S);
        A += (double)rS;
        B += (double)((float)D * rS * rS);
        if (lane == 0) {  // history entry t+1 = (A, B) after step t (also of the step that ends the loop: an open start cell's stamp is 1)
            hist_st<kHistLds>(&hist[2 * (t + 1)], A);
            hist_st<kHistLds>(&hist[2 * (t + 1) + 1], B);
        }
        const bool goal_step = s == gidx;
        const bool last_step = t == n_steps - 1;
        if (goal_step && last_step && extra <= 0) {  // the step that ends the batch loop: its softmax counted, nothing follows
            pend = false;
            break;
        }
        // expansion of s (:222-249): lanes 0..7 relax the neighbours, lane 8 closes s (the goal stays open, :224)
        const int r = s / d.W, c = s - r * d.W;
        const int nr = r + dr, nc = c + dc;
        const bool inb = is_nb & ((unsigned)nr < (unsigned)d.H) & ((unsigned)nc < (unsigned)d.W);
        const int il = inb ? s + noff : s;
        const float gs = st_ld<kGlobal>(&g[s]), cs = st_ld<kGlobal>(&cst[s]);
        const float gl = st_ld<kGlobal>(&g[il]), cl = st_ld<kGlobal>(&cst[il]);
        const float Gl = st_ld<kGlobal>(&G[il]);
        const int tl = (int)st_ld<kGlobal>(&t0[il]);
        const int rl = il / d.W, cc = il - rl * d.W;
        const float hh = d.omg * (h0(il, rl, cc, goal_r, goal_c) + cl);
        const float g2 = gs + cs;
        const bool upd = inb & (gl > g2);
        const bool was_open = fabsf(gl) < NASTAR_POS_INF;
        // lane 8 at the goal's last re-selection of a budget-truncated lock-step log: the goal stays open with the same v, but its interval with
        // G = 0 ends here and one with the upstream value begins (D gains v * G_up)
        const bool restore = (lane == 8) & goal_step & (t == t_restore);
        const bool flushing = (upd & was_open) | ((lane == 8) & !goal_step) | restore;
        const float v_old = bwdr_v<kFastDiv>(d, gl, hh, rcp_sqrtW);
        const float v_new = bwdr_v<kFastDiv>(d, g2, hh, rcp_sqrtW);
        if (upd | flushing) {
            const double dS = (upd ? (double)v_new : 0.0) - ((flushing & !restore) ? (double)v_old : 0.0);
            const double dD = (upd ? (double)(Gl * v_new) : 0.0) - (flushing ? (double)(Gl * v_old) : 0.0) + (restore ? (double)(goal_up * v_old) : 0.0);
            // ds_add_f64 issued directly: for a wave-uniform address hipcc's atomic optimizer would first reduce the lanes in a
            // scalar loop (one iteration per active lane); the LDS unit serialises the <= 9 same-address adds much faster
            const uint32_t sda = (uint32_t)(uintptr_t)sd;
            asm volatile("ds_add_f64 %0, %1\n\tds_add_f64 %0, %2 offset:8" ::"v"(sda), "v"(dS), "v"(dD) : "memory");
        }
        if (upd) {
            st_st<kGlobal>(&g[il], g2);
            st_st<kGlobal>(&t0[il], (stamp_t)(t + 1));
        }
        if ((lane == 8) & !goal_step) st_st<kGlobal>(&g[s], NASTAR_NEG_INF);
        if (restore) {
            st_st<kGlobal>(&G[s], goal_up);
            st_st<kGlobal>(&t0[s], (stamp_t)(t + 1));
        }
        // close the interval of every cell that left the open list or was re-keyed: load its opening stamp, consume next step
        // (the start cell closed by step 0 carries stamp 1 = this step's own entry: an empty interval, nothing to add)
        pend = flushing & (tl != t + 1);
        pv = v_old;
        pG = Gl;
        pcell = il;
        pA = A;
        pB = B;
        if (pend) {
            pA0 = hist_ld<kHistLds>(&hist[2 * tl]);
            pB0 = hist_ld<kHistLds>(&hist[2 * tl + 1]);
        }
        wave_order();
        if (goal_step && last_step) {  // extra > 0: `extra` more identical steps on the open list left by the goal's own expansion
            goal_fixed_point = true;
            break;
        }
    }
    global_step_fence();
    if (pend) {
        const float dA = (float)(pA - pA0), dB = (float)(pB - pB0);
        unsafeAtomicAdd(&gout[pcell], (a.kfac * pv) * (pG * dA - dB));
    }
    wave_sync();
    if (goal_fixed_point) {
        const double S = sd[0], D = sd[1];
        const float rS = __builtin_amdgcn_rcpf((float)S);
        A += (double)extra * (double)rS;
        B += (double)extra * (double)((float)D * rS * rS);
    }
    if constexpr (kGlobal) {  // the sweep launch closes the intervals of the cells still on the open list
        if (lane == 0) {
            *reinterpret_cast<double*>(hdr + 2) = A;
            *reinterpret_cast<double*>(hdr + 4) = B;
        }
        return;
    }
    // cells still on the open list: close their intervals at the final (A, B)
    for (int i = lane; i < d.HW; i += 64) {
        const float gi = st_ld<kGlobal>(&g[i]);
        if (fabsf(gi) < NASTAR_POS_INF) {
            const int ti = (int)st_ld<kGlobal>(&t0[i]);
            const double A0 = hist_ld<kHistLds>(&hist[2 * ti]);
            const double B0 = hist_ld<kHistLds>(&hist[2 * ti + 1]);
            const int ri = i / d.W, ci = i - ri * d.W;
            const float hh = d.omg * (h0(i, ri, ci, goal_r, goal_c) + st_ld<kGlobal>(&cst[i]));
            const float v = bwdr_v<kFastDiv>(d, gi, hh, rcp_sqrtW);
            const float dA = (float)(A - A0), dB = (float)(B - B0);
            unsafeAtomicAdd(&gout[i], (a.kfac * v) * (st_ld<kGlobal>(&G[i]) * dA - dB));
        }
    }
