// np_filter_emit.inc -- stages 5 and 6 of a narrow-phase work item, as TEXT: thin the contacts (greedy normal clusters, hull
// of each; contacts.py:97-158) and write the kept ones, in ascending face order, to the pair's output slots.
// Included inside narrow_pair (narrowphase.hip; the lean kernel's register allocation depends on this code sitting in that
// function as written) and as the body of filter_and_emit (np_common.h) for the round-based neural narrow phase.
// Expects in scope: G, W, S, item, sc, np, dp, tid, ncon, over, cface, kface, cstate, cb + CB(f, k), MC, pc_count, STAMP(i) (np_common.h).
// On entry the candidate scratch holds, for contacts k < ncon: kface[k] and the contact fields of CandField (np_common.h):
// barycentrics, normal, p1, p2, penetration.
    STAMP(4);
    // ---- 5. filter: greedy normal clusters, hull of each (contacts.py:97-158) -------------------
    int nkeep = 0;
    unsigned keptbits = 0u;
    if (ncon <= 1) {
        if (tid == 0) cstate[0] = -2;  // kept
        nkeep = ncon;
    } else {
        // The state of every contact lives in LDS bytes while the clusters are formed (a wavefront-sized group needs
        // ncon <= HCAP anyway; a workgroup falls back to the global array beyond its LDS capacity), and the six
        // numbers a contact contributes (normal, p1) are fetched in one batch per round: every dependent global
        // round trip costs a microsecond here.
#if !DSS_ALL_SHAPES
        // the mask of kept contacts below holds 32 rounds of the group: a pair with more contacts than that (in clusters that
        // each stay below HCAP, or bit 2 is raised anyway) is a capacity error of the lean variant like a cluster beyond HCAP
        if (ncon > 32 * G::BT) { over |= 2; ncon = 32 * G::BT; }
#endif
        const bool lds_state = ncon <= G::HCAP;
        if (!lds_state && G::BT == 64) return 1;
        auto get_state = [&](int k) -> int { return lds_state ? (int)S.cst[k] : cstate[k]; };
        auto set_state = [&](int k, int v) { if (lds_state) S.cst[k] = (unsigned char)v; else cstate[k] = v; };
        // (NP_PRESTATE: the including stage 4 has left this state in S.cst already, with the normal still in registers)
#if defined(NP_PRESTATE)
        if (!lds_state)
#endif
        for (int k = tid; k < ncon; k += G::BT) {
            const double nn = t_sqrt(CB(F_NORMAL, k) * CB(F_NORMAL, k) + CB(F_NORMAL + 1, k) * CB(F_NORMAL + 1, k) + CB(F_NORMAL + 2, k) * CB(F_NORMAL + 2, k));
            set_state(k, nn > 1e-12 ? 0 : 255);
        }
        G::sync();
        for (int cl = 1; cl <= ncon; ++cl) {
            int mine = -1;
            for (int k = tid; k < ncon; k += G::BT) if (get_state(k) == 0) { mine = k; break; }
            const int seed = block_argmin(mine >= 0 ? (double)mine : INFINITY, mine, S);
            if (seed < 0) break;
            const double sn[3] = {CB(F_NORMAL, seed), CB(F_NORMAL + 1, seed), CB(F_NORMAL + 2, seed)};
            // gather the cluster (ascending) into the hull scratch
            int m = 0;
            for (int base = 0; base < ncon; base += G::BT) {
                const int k = base + tid;
                int in = 0;
                double p1v[3] = {0.0, 0.0, 0.0};
                if (k < ncon && get_state(k) == 0) {
                    const double nk[3] = {CB(F_NORMAL, k), CB(F_NORMAL + 1, k), CB(F_NORMAL + 2, k)};
                    for (int i = 0; i < 3; ++i) p1v[i] = CB(F_P1 + i, k);
                    const double d = fmin(nk[0] * sn[0] + nk[1] * sn[1] + nk[2] * sn[2], 1.0);
                    // acos(d) < 1e-2 (contacts.py:112): decided by d against cos(1e-2) wherever that is safe (a margin of
                    // 1e-12 in d is 1e-10 rad, a million times acos' rounding); the arc cosine itself only in between
                    constexpr double C01 = 0.99995000041666528;
                    in = d > C01 + 1e-12 ? 1 : (d < C01 - 1e-12 ? 0 : (int)(acos(d) < 1e-2));
                }
#if DSS_ALL_SHAPES
                const int slot = compact_slot(in, m, S);
                if (slot >= 0) {
                    set_state(k, 3);     // member of the cluster being thinned
                    if (slot < G::HCAP) { S.hidx[slot] = k; for (int i = 0; i < 3; ++i) S.hp[3 * slot + i] = p1v[i]; }
                }
            }
            G::sync();
            if (m <= G::HCAP) {
                if (cluster_hull(S, HullLds<G>{&S}, m, W.eps)) return 1;
                for (int j = tid; j < m; j += G::BT) set_state(S.hidx[j], S.hflag[j] ? 2 : 1);
            } else {
                // more points than the LDS scratch holds (a level-set mesh lying flat on its neighbour: every face of that
                // side is a contact with the same normal): gather the members again, into the global candidate scratch
                if (G::BT == 64) return 1;
                m = 0;
                for (int base = 0; base < ncon; base += G::BT) {
                    const int k = base + tid;
                    const int in = k < ncon && get_state(k) == 3;
                    const int slot = compact_slot(in, m, S);
                    if (slot >= 0) { cface[slot] = k; for (int i = 0; i < 3; ++i) CB(F_HULL_P + i, slot) = CB(F_P1 + i, k); }
                }
                G::sync();
                const HullGlobal P{cb, MC};
                cluster_hull(S, P, m, W.eps);
                for (int j = tid; j < m; j += G::BT) set_state(cface[j], P.getf(j) ? 2 : 1);
            }
            G::sync();
        }
#else
                const int slot = compact_slot(in, m, S);
                if (slot >= 0) {
                    set_state(k, 1);
                    if (slot < G::HCAP) { S.hidx[slot] = k; for (int i = 0; i < 3; ++i) S.hp[3 * slot + i] = p1v[i]; }
                }
            }
            G::sync();
            if (m > G::HCAP) { if (G::BT == 64) return 1; over |= 2; m = G::HCAP; }
            if (cluster_hull(S, HullLds<G>{&S}, m, W.eps) == 2) over |= 128;      // (needs the exact hull of the full variants)
            for (int j = tid; j < m; j += G::BT) if (S.hflag[j]) set_state(S.hidx[j], 2);
            G::sync();
        }
#endif
        for (int k = tid, r = 0; k < ncon; k += G::BT, ++r) {
            const int kept = get_state(k) == 2;
#if DSS_ALL_SHAPES
            if (r < 32)
#endif
            keptbits |= (unsigned)kept << r;     // round r of this thread: the final stage walks the same (round, thread) grid
            nkeep += kept;
        }
        nkeep = (int)(block_sum((double)nkeep, S) + 0.5);
    }

    STAMP(5);
    // ---- 6. the kept contacts (geometry from stage 4), in ascending face order --------------------
    // (the reference emits cluster by cluster in Qhull's vertex order, which is implementation
    //  defined; contact sets of a pair are compared as sets, SURVEY.md §7)
    int nout = 0;
    const int MP = W.max_pc;
    int *pf = W.pc_face + ((size_t)sc * np + dp) * MP;
    double *pabc = W.pc_abc + ((size_t)sc * np + dp) * 3 * MP, *pg = W.pc_geom + ((size_t)sc * np + dp) * 10 * MP;
    if (ncon <= 1) {
        if (tid == 0) {
            pf[0] = kface[0];
            for (int i = 0; i < 3; ++i) { pabc[(size_t)i * MP] = CB(F_CABC + i, 0); pg[(size_t)i * MP] = CB(F_NORMAL + i, 0); pg[(size_t)(3 + i) * MP] = CB(F_P1 + i, 0); pg[(size_t)(6 + i) * MP] = CB(F_P2 + i, 0); }
            pg[(size_t)9 * MP] = CB(F_PEN, 0);
        }
        nout = 1;
    } else {
        for (int base = 0, r = 0; base < ncon; base += G::BT, ++r) {
            const int k = base + tid;
            // beyond 32 rounds (more than 32 x group size contacts: a level-set face lying flat) the bit mask is full and the
            // state array, which such a count keeps in global memory, is read instead
#if DSS_ALL_SHAPES
            const int flag = (k < ncon) && (r < 32 ? (int)((keptbits >> r) & 1u) : (cstate[k] == 2));
#else
            const int flag = (k < ncon) && ((keptbits >> r) & 1u);     // (the lean variant stops at HCAP contacts per cluster and 32 rounds per pair)
#endif
            if (!G::any(flag)) continue;
            const int slot = compact_slot(flag, nout, S);
            if (slot >= 0 && slot < MP) {
                pf[slot] = kface[k];
                for (int i = 0; i < 3; ++i) {
                    pabc[(size_t)i * MP + slot] = CB(F_CABC + i, k);
                    pg[(size_t)i * MP + slot] = CB(F_NORMAL + i, k); pg[(size_t)(3 + i) * MP + slot] = CB(F_P1 + i, k); pg[(size_t)(6 + i) * MP + slot] = CB(F_P2 + i, k);
                }
                pg[(size_t)9 * MP + slot] = CB(F_PEN, k);
            }
        }
        if (nout > MP) { over |= 4; nout = MP; }
    }
    if (tid == 0) { *pc_count = nout; if (over) atomicOr(W.overflow + sc, over); }
    STAMP(6);
    return 0;
