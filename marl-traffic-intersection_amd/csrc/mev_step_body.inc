// mev_step_body.inc -- the body of one fused step of a workgroup's envs
// (mev_kernels.hip): included as the body of k_step, and inside a lambda in
// k_serve's loop (its returns then end the step, not the server).  Expects in
// scope: the template parameters TRAFFIC, TAB, NM, KM, PK, SPLIT, ESPLIT, P1, NC, WC and
// pp (const SimParams*), in (StepInputs), out (Outputs).  Kept textually in the
// kernel: passing the step to an inlined function changed k_step's code (1.2 %
// slower at config 3, profiles/r3_ab_step_body.txt).  An includer may define
// MEV_STEP_BODY_AFTER_CARS: statements that run after cars_post / deal_append and before
// the LiDAR, with the car part's CarsCtx `cx` in scope (k_rollout's frame skip returns
// there from a sub-step that needs no cast); undefined, the body is what it was.
    static_assert(!SPLIT || !TRAFFIC || ESPLIT, "split waves with traffic: the early split");
    static_assert(!WC || (!TRAFFIC && !TAB && NM > 0 && PK == 1 && !SPLIT && P1 >= WAVE && NC > 0),
                  "the world at compile time: one wave per env, the counts at compile time, no table");
    const SimParams& p = *pp;
    extern __shared__ __align__(16) unsigned char step_lds[];
    const int wv = SPLIT ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    // PK envs per wave (few agents per env): envs e .. e + PK - 1, see cars_pre
    int npc_cls = kDealClasses - 1;  // (the env's NPC class in the deal; unknown: every slot)
    const int e = (TRAFFIC && (in.deal & 1)) ? deal_env(p, in.deal_ring, (int)blockIdx.x, 1, 0, &npc_cls)
                                             : xcd_env((int)blockIdx.x, (int)gridDim.x) * PK;
#if defined(MEV_STAMPS_R)
    STAMP_RAW(0);
#endif
    QSTAMP(0);
    constexpr int KF = TRAFFIC ? KM : 0;  // NPC obstacle slots of the compile-time layout
    // the car phase's segments by lane (lidar_body): <= 8 agents per pool, <= 8 boxes per wave
    constexpr bool SEGL = NM == 8 && KF == 0;
    // agents per env at compile time (0: p.N): NC, or one with the one-ego layout (N >= 1)
    constexpr int NCE = NM == 1 ? 1 : NC;
    const StepLayout sl = step_layout_t<NM, KF>(p);
    // NM = 0 (runtime layout) also runs handles whose cars have other sizes (p.dims)
    constexpr bool DIMS = NM == 0;
    using NLT = NpcLDST<KM, DIMS>;
    CarsLDS el = NM ? carve_cars_lds(step_lds, NM, KF) : carve_cars_lds(step_lds, p.N, cars_k(p), DIMS);
    el.head = reinterpret_cast<float*>(step_lds + sl.head);
    el.rel = reinterpret_cast<float*>(step_lds + sl.rel);
    el.envw = reinterpret_cast<int32_t*>(step_lds + sl.envw);
    if constexpr (!TRAFFIC && NM > 0) {
        static_assert(NM == 0 || FixedLayout<(NM ? NM : 1), 0>::lay.bytes >= kWinBytes, "LDS path windows");
        el.win = reinterpret_cast<float4*>(step_lds + sl.lidar);
    }
    // (the traffic early split: one NPC area per env of the workgroup)
    __shared__ typename std::conditional<TRAFFIC, NLT, char>::type nl_storage[(TRAFFIC && ESPLIT) ? PK : 1];
    NLT* nl = nullptr;
    if constexpr (TRAFFIC) nl = &nl_storage[0];
    __builtin_amdgcn_s_setprio(kPrioCars);
    if constexpr (TRAFFIC && ESPLIT) {
        // The traffic early split: PK envs of one ego each per workgroup, wave j < PK
        // the car wave of env j (NPC phase, kinematics, status, SAT, respawn, obstacle
        // table; barrier B; cars_post), wave PK their LiDAR wave: the egos' poses after
        // Car::update and the road march beside the car waves (the reference's ego
        // update and road march never read an NPC: TrafficFlow.cpp:49-196 ignores the
        // egos, IntersectionEnv.cpp:140-163 updates them after the traffic), then
        // after barrier B the respawned egos' beams again and every ego's car pairs
        // against its own env's table.  PK + 1 waves per PK envs (kTsplitEnvs = 2: 6 waves
        // per SIMD, <= 85 VGPRs, at config 4).
        static_assert(SPLIT && NM == 1 && KF > 0, "traffic early split: one ego per env, compile-time layout");
        constexpr int REG = FixedLayout<1, KF>::lidar;  // one env's car LDS, beam offsets and flags
        const int lane = threadIdx.x & (WAVE - 1);
        const int b = (int)blockIdx.x;
        if (wv < PK) {
            // (its own env only: four envs' deal lookups in every car wave cost 4.6 k cycles of
            // its load phase, profiles/r5_q_cfg4_tsplit.txt)
            int cls = kDealClasses - 1;
            const int ej = (in.deal & 1) ? deal_env(p, in.deal_ring, b, PK, wv, &cls) : xcd_env(b, (int)gridDim.x) * PK + wv;
            unsigned char* rb = step_lds + wv * REG;
            CarsLDS elj = carve_cars_lds(rb, 1, KF);
            elj.head = reinterpret_cast<float*>(rb + sl.head);
            elj.rel = reinterpret_cast<float*>(rb + sl.rel);
            elj.envw = reinterpret_cast<int32_t*>(rb + sl.envw);
            NLT* nlj = &nl_storage[wv];
            __builtin_amdgcn_s_setprio(kPrioTsplitCars);
            CarsCtx cx = cars_pre<true, true, NLT, 1, false, true, false, true, NCE>(p, in, out, ej, elj, nlj, cls);
            cars_post<true, true, NLT, 1, false, NCE>(p, out, ej, elj, nlj, cx);
            deal_append<true>(p, in, cx, ej);
#if defined(MEV_STAMPS_Q)
            QSTAMP(7);
            if (lane == 0)
                for (int q = 0; q < 8; ++q) p.debug[ej * 8 + q] = mev_qst[wv * 8 + q];
#endif
            return;
        }
        __builtin_amdgcn_s_setprio(kPrioTsplitLidar);
        int es[PK];  // the workgroup's envs
#pragma unroll
        for (int j = 0; j < PK; ++j)
            es[j] = (in.deal & 1) ? deal_env(p, in.deal_ring, b, PK, j) : xcd_env(b, (int)gridDim.x) * PK + j;
        unsigned char* lbase = step_lds + PK * REG;
        constexpr LidarLayout lay = lidar_layout_beams(PK, PK * kTsplitRays, KF, false);
        float* rel0 = reinterpret_cast<float*>(step_lds + sl.rel);
        for (int bb = lane; bb < p.R; bb += WAVE) rel0[bb] = gmem(p.rel_angles)[bb];
        // slot (lane) j < PK: env j's ego loaded and run through phase 1 into its env's LDS
        // (kinematics, path index, status: ts_ego_phase) while the car waves run the NPC
        // phase; the road march starts from those poses
        const unsigned long long am = ts_ego_phase<PK, KF>(p, in, step_lds, REG, es, lane);
        const bool on = lane < PK;
        const bool alive = ((am >> lane) & 1ull) != 0;
        int ee = es[0];
#pragma unroll
        for (int j = 1; j < PK; ++j) ee = lane == j ? es[j] : ee;
        // a dead ego's LiDAR block is zero (:425-427)
        for (unsigned long long dm = ballot(on && !alive); dm; dm &= dm - 1ull) {
            const int g = __builtin_amdgcn_readlane(ee, __builtin_ctzll(dm));
            if (out.lidar_u8) {
                for (int bb = lane; bb < p.lidar_slots; bb += WAVE)
                    out.lidar_u8[(size_t)g * p.lidar_slots + bb] = (uint8_t)kLidarCodeDead;
            } else {
                for (int bb = lane; bb < p.lidar_slots; bb += WAVE) out.obs[(size_t)g * out.obs_ld + OBS_HEAD + bb] = 0.0f;
            }
        }
        float4* ag = reinterpret_cast<float4*>(lbase + lay.ag);
        if (alive) {
            const CarsLDS elp = carve_cars_lds(step_lds + lane * REG, 1, KF);
            ag[lane_rank(am)] = make_float4(elp.x[0], elp.y[0], elp.h[0], __int_as_float(ee));
        }
        wave_lds_sync();
        const CarsLDS el0 = carve_cars_lds(step_lds, 1, KF);
        LidarSrcLdsEnvs<PK> src{el0, REG, rel0, {}};
#pragma unroll
        for (int j = 0; j < PK; ++j) src.env[j] = es[j];
        const int nal = __popcll(am);
        lidar_body<TAB, kEsplitIlp, LidarSrcLdsEnvs<PK>, LIDAR_NPR, true, 1, P1, false, false, kRoadBoundTraffic>(
            p, out, src, PK, 0, nal, lane, lbase, lay, 0ull, am);
        __syncthreads();  // barrier H: the car waves take their egos from here (after their NPC phase)
        __syncthreads();  // barrier B: the car waves' obstacle tables, candidate masks and respawns
        // respawned egos: their spawn poses into ag[] and their beams marched again
        const int li = on ? lane : 0;
        const bool rs = alive && (reinterpret_cast<const int32_t*>(step_lds + li * REG + sl.envw)[6] & 1) != 0;
        const unsigned long long rl = ballot(rs);
        unsigned long long redo = 0ull;
        if (rl != 0ull) {
            if (rs) {
                const CarsLDS elr = carve_cars_lds(step_lds + li * REG, 1, KF);
                ag[lane_rank(am)] = make_float4(elr.x[0], elr.y[0], elr.h[0], __int_as_float(ee));
            }
            for (unsigned long long m = rl; m; m &= m - 1ull) {
                const int i = __builtin_ctzll(m);
                redo |= 1ull << __popcll(am & ((1ull << i) - 1ull));
            }
            wave_lds_sync();
        }
        __builtin_amdgcn_s_setprio(kPrioEsplitCarPhase);
        lidar_body<TAB, kEsplitIlp, LidarSrcLdsEnvs<PK>, LIDAR_NPR, true, 2, P1, false, false, kRoadBoundTraffic>(
            p, out, src, PK, 0, nal, lane, lbase, lay, redo, am);
        return;
    } else if constexpr (ESPLIT) {
        static_assert(SPLIT && !TRAFFIC && NM > 0, "early split without traffic: two waves");
        const int lane = threadIdx.x & (WAVE - 1);
        const int NE = NCE ? NCE : p.N;
        const int g0 = e * NE;
        // the wave's agent slots: PK envs of N agents (consecutive in the SoA), one LiDAR pool
        const int NS = PK == 1 ? NE : (p.E - e < PK ? p.E - e : PK) * NE;
        unsigned char* lbase = step_lds + sl.lidar;
        const LidarLayout lay = FixedLayout<(NM ? NM : 1), 0>::lay;
        if (wv == 0) {
            // the car part (its path windows through VGPRs: the LiDAR wave owns the LiDAR
            // area from the start), barrier B at the end of cars_pre
            __builtin_amdgcn_s_setprio(kPrioEsplitCars);
            CarsCtx cx = cars_pre<false, true, NLT, PK, false, true, false, false, NCE>(p, in, out, e, el, nl);
            cars_post<false, true, NLT, PK, false, NCE>(p, out, e, el, nl, cx);
        } else {
            __builtin_amdgcn_s_setprio(kPrioEsplitRoad);
            // the beam offsets (this wave stages them in the early split) and, lane i < N,
            // agent i's pose after Car::update exactly as cars_pre computes it (an env
            // whose previous step ended starts from its spawns; a dead agent keeps its
            // pose): the road march needs nothing else from the car part
            for (int b = lane; b < p.R; b += WAVE) el.rel[b] = gmem(p.rel_angles)[b];
            const bool on = lane < NS;
            const int il = on ? lane : 0;
            const int ee = PK == 1 ? e : e + il / NE;  // the slot's env
            const uint32_t ug = (uint32_t)(g0 + il);
            const bool pend = ldu(gmem(p.pending_reset), (uint32_t)ee) != 0;
            const int route_l = ldu(egoi(p, EF_ROUTE), ug);
            Kin k{ldu(egof(p, EF_X), ug), ldu(egof(p, EF_Y), ug), ldu(egof(p, EF_V), ug), ldu(egof(p, EF_H), ug),
                  ldu(egof(p, EF_ACC), ug), ldu(egof(p, EF_STEER), ug)};
            bool alive = ldu(gmem(p.ego.alive), ug) != 0;
            const float a0 = ldu(gmem(in.actions), 2 * ug), a1 = ldu(gmem(in.actions), 2 * ug + 1);
            if (in.auto_reset && pend) {
                const int rid = reset_route(p, in.rng_counter, ee, PK == 1 ? il : il - (ee - e) * NE, route_l);
                k = Kin{gmem(p.rt.spawn)[3 * rid], gmem(p.rt.spawn)[3 * rid + 1], 0.0f, gmem(p.rt.spawn)[3 * rid + 2],
                        0.0f, 0.0f};
                alive = true;
            }
            {
                Kin ku = k;
                float sH, cH;
                car_update_heading(ku, a0, a1, in.dt);
                sincosf(alive ? ku.h : k.h, &sH, &cH);
                car_update_move(ku, cH, sH);
                if (alive) k = ku;
            }
            alive = on && alive;
            const unsigned long long am = ballot(alive);
            float4* ag = reinterpret_cast<float4*>(lbase + lay.ag);
            if (alive) ag[lane_rank(am)] = make_float4(k.x, k.y, k.h, __int_as_float(g0 + il));
            wave_lds_sync();
            lidar_body<TAB, kEsplitIlp, LidarSrcLds, LIDAR_NPR, true, 1, P1, false, SEGL, kRoadBoundStep>(
                p, out, LidarSrcLds{el, g0}, NS, g0, NS, lane, lbase, lay, 0ull, am);
            __syncthreads();  // barrier B: the car part's obstacle table, candidate masks and respawns
            // respawned egos: their spawn poses into ag[] and their beams marched again
            const unsigned rmask = (unsigned)el.envw[6];
            const bool rs = alive && lane < 32 && ((rmask >> (lane & 31)) & 1u);
            const unsigned long long rl = ballot(rs);
            unsigned long long redo = 0ull;
            if (rl != 0ull) {
                if (rs) ag[lane_rank(am)] = make_float4(el.x[lane], el.y[lane], el.h[lane], __int_as_float(g0 + lane));
                for (unsigned long long m = rl; m; m &= m - 1ull) {
                    const int i = __builtin_ctzll(m);
                    redo |= 1ull << __popcll(am & ((1ull << i) - 1ull));
                }
                wave_lds_sync();
            }
            __builtin_amdgcn_s_setprio(kPrioEsplitCarPhase);
            lidar_body<TAB, kEsplitIlp, LidarSrcLds, LIDAR_NPR, true, 2, P1, false, SEGL, kRoadBoundStep>(
                p, out, LidarSrcLds{el, g0}, NS, g0, NS, lane, lbase, lay, redo, am);
        }
        return;
    }
    if constexpr (!(TRAFFIC && ESPLIT)) {  // (the traffic early split returned above)
    CarsCtx cx{};
    if (wv == 0) cx = cars_pre<TRAFFIC, true, NLT, PK, (!TRAFFIC && NM > 0), false, DIMS, false, NCE, false, WC>(p, in, out, e, el, nl, npc_cls);
    if (SPLIT) __syncthreads();
    else wave_lds_sync();
#if !defined(MEV_EXP_STOP) || MEV_EXP_STOP != 0  // timing-only stop0: the car part without cars_post
    if (wv == 0) {
        cars_post<TRAFFIC, true, NLT, PK, DIMS, NCE, false, (WC ? P1 : 0)>(p, out, e, el, nl, cx);
        wave_lds_sync();
    }
#endif
    deal_append<TRAFFIC>(p, in, cx, e);
#if defined(MEV_STEP_BODY_AFTER_CARS)  // an includer's hook after the car part (k_rollout's frame skip); else nothing
    MEV_STEP_BODY_AFTER_CARS
#endif
#if defined(MEV_EXP_STOP) && MEV_EXP_STOP == 0  // (stop0 keeps the deal: the env order stays the product's)
    return;
#endif
    if (SPLIT && wv == 0) return;  // wave 1 runs the LiDAR
#if defined(MEV_EXP_STOP) && MEV_EXP_STOP == 1  // timing-only: the car part alone
    return;
#endif
    // agent slots of this wave and its LiDAR pools of <= 512 beams (one at config 3)
    const int NEC = NCE ? NCE : p.N;
    const int NS = PK == 1 ? NEC : (p.E - e < PK ? p.E - e : PK) * NEC;
    int G = 512 / (p.R > 0 ? p.R : 1);
    G = G < 1 ? 1 : (G < NS ? G : NS);
    if (PK == 1) G = (NCE > 0 && P1 >= WAVE) ? step_pool_n(NCE, P1) : step_pool(p);  // (counts at compile time: a constant)
    const LidarLayout lay = NM ? FixedLayout<(NM ? NM : 1), KF>::lay : lidar_layout(G, p.R, lidar_cand_max(p), false);
    unsigned char* lbase = step_lds + sl.lidar;
    const int lane = threadIdx.x & (WAVE - 1);
    const int g0 = e * NEC;
    for (int j0 = 0; j0 < NS; j0 += G) {  // pools of G agents (one at config 3)
        if (j0 > 0) wave_lds_sync();
        if (j0 > 0) __builtin_amdgcn_s_setprio(kPrioLidar);  // each further pool (cars and LiDAR start at one level)
        const int na = NS - j0 < G ? NS - j0 : G;
        lidar_body<TAB, kPhase1Ilp, LidarSrcLds, LIDAR_NPR, true, 0, P1, WC, SEGL,
                   (TRAFFIC ? kRoadBoundTraffic : kRoadBoundStep)>(
            p, out, LidarSrcLds{el, g0}, G, g0 + j0, na, lane, lbase, lay);
    }
#if defined(MEV_STAMPS_Q)
    QSTAMP(7);
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 8; ++q) p.debug[e * 8 + q] = mev_qst[wv * 8 + q];
#endif
#if defined(MEV_STAMPS_R)  // slot 7: end of the wave (low 40 bits) | where it ran (HW_ID[15:0], XCC_ID[2:0]) << 40
    if (!SPLIT || wv == 1) {
        const unsigned long long t = __builtin_amdgcn_s_memrealtime() & ((1ull << 40) - 1);
        const unsigned hw = __builtin_amdgcn_s_getreg((15 << 11) | 4) & 0xffffu;
        const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;
        if (lane == 0) p.debug[e * 8 + 7] = t | ((unsigned long long)(hw | (xcc << 16)) << 40);
    }
#endif
    }
