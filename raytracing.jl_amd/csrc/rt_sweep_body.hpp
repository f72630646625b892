// rt_sweep_body.hpp — the body of the sweep kernels, included by rt_sweep.hip inside k_sweep (REPRO = false) and inside its sibling
// k_sweep_repro (REPRO = true, LDS = false): one text, two kernels, and k_sweep compiles to the instructions it had as a kernel of
// its own (called as an inlined device function it did not).  Expects the template flags STAGED, GP, LDS, ELLROWS, P1, LS, the
// constant REPRO and the kernel argument `DSweep a` in scope; rt_sweep.hip's head comment describes what it does.
// A third kernel, k_sweep_iface (rt_sweep_iface.hip), includes it with the constant IFACE = true (false in the two above, whose
// instructions stay what they were): the partial currents between cell regions, `if constexpr (IFACE)` below.
// A fourth, k_sweep_void (rt_sweep_void.hip), includes it with the constant VOID = true (false in the three above, whose instructions
// stay what they were): in a cell whose Σt is 0 the tally is the track length w ψ ℓ, `if constexpr (VOID)` below.
    static_assert(STAGED || !ELLROWS, "ℓ rows belong to the staging rows");
    static_assert(!(REPRO && LDS), "the reproducible tallies keep no LDS copy");
    static_assert(!IFACE || (STAGED && ELLROWS && !REPRO), "the region currents are tallied over (ℓ, cell) rows, by atomics");
    static_assert(!(P1 && LS), "linear source with first-moment scattering is not built");
    static_assert(!VOID || (STAGED && ELLROWS && !REPRO && !IFACE && !LS), "the void tally is built over (ℓ, cell) rows, by atomics, flat or with first moments");
    constexpr bool AN = P1 || LS;        // three tallies and two ratios per component
    constexpr int NT = AN ? 3 : 1;       // tallies per component
    constexpr int NH = LS ? 2 * GP + 2 : (P1 ? 2 * GP : 1);  // ratios of a pass (one unused slot when isotropic); LS: + the cell's centroid
    extern __shared__ __attribute__((aligned(16))) unsigned char sweep_smem[];
    double *hist = reinterpret_cast<double *>(sweep_smem);  // [n_cells * NT * GP] when LDS
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform, and known to be
    // IFACE: the workgroup's table of the pass, S[from][to][g] with from, to in 0 .. R (R: outside the track), behind the φ copy
    [[maybe_unused]] double *itab = nullptr;
    [[maybe_unused]] int R1 = 1, ntab = 0;
    if constexpr (IFACE) {
        itab = hist + (LDS ? a.n_cells * (NT * GP) : 0);
        R1 = a.if_R + 1; ntab = R1 * R1 * GP;
    }
    if (LDS)
        for (int c = threadIdx.x; c < a.n_cells * (NT * GP); c += blockDim.x) hist[c] = 0.0;
    if constexpr (IFACE)
        for (int c = threadIdx.x; c < ntab; c += blockDim.x) itab[c] = 0.0;
    if (LDS || IFACE) __syncthreads();
    // a sweep wave = (march wave, direction).  The march waves are ordered longest first and the sweep is bound by
    // instruction issue, so the waves are dealt to the workgroups round-robin: wave k of workgroup b takes sweep wave
    // k * gridDim + b — every workgroup gets the same mix of long and short tracks and all finish together (contiguous
    // blocks of 16 sweep waves left the CU with the longest tracks working 1.6x longer than the average one).
    const int64_t sw = (int64_t)wib * gridDim.x + blockIdx.x;
    const int64_t mw = sw >> 1;
    const int dir = (int)(sw & 1);
    if (mw < a.n_waves) {
        const int64_t slot = mw * 64 + lane;
        const bool have = slot < a.n;
        const int32_t u = have ? a.perm[slot] : 0;
        const int32_t cnt = have ? a.counts[u] : 0;
        int32_t mc = cnt;
        for (int o = 32; o > 0; o >>= 1) {
            const int32_t v = __shfl_xor(mc, o, 64);
            mc = v > mc ? v : mc;
        }
        const int maxcnt = __builtin_amdgcn_readfirstlane(mc);
        const double w = !have ? 0.0 : (a.w ? a.w[u] : a.delta_s[a.azim[u] - 1]);
        // P1: the traversal's direction cosines d (cos ϕ, sin ϕ) and the weight times them (0 for a lane without a track)
        double dcs = 0.0, dsn = 0.0, wcs = 0.0, wsn = 0.0;
        if constexpr (AN) {
            const double c0 = have ? a.cs[u] : 0.0, s0 = have ? a.sn[u] : 0.0;
            dcs = dir ? -c0 : c0; dsn = dir ? -s0 : s0;
            wcs = w * dcs; wsn = w * dsn;
        }
        // LS: the traversal's entry point (first record's p forward, last record's q backward) and the path length behind the lane
        double ex = 0.0, ey = 0.0, srun = 0.0;
        if constexpr (LS) {
            if (have) { ex = a.ends[(int64_t)u * 4 + 2 * dir]; ey = a.ends[(int64_t)u * 4 + 2 * dir + 1]; }
        }
        const int64_t off = (!STAGED && have) ? a.offsets[u] : 0;
        const int64_t pbase = ((int64_t)dir * a.n + u) * a.G + a.g0;
        const int ng = a.ng;
        double psi[GP];
#pragma unroll
        for (int g = 0; g < GP; ++g) psi[g] = (have && g < ng) ? a.psi_in[pbase + g] : 0.0;
        // IFACE: the region of the lane's previous record (R before its first one), and the add of w ψ to the table's [from][to]
        [[maybe_unused]] int32_t rprev = 0;
        if constexpr (IFACE) rprev = a.if_R;
        [[maybe_unused]] auto iface_add = [&](const int32_t from, const int32_t to) {
#pragma unroll
            for (int g = 0; g < GP; ++g)
                if (g < ng) atomicAdd(&itab[(from * R1 + to) * GP + g], w * psi[g]);  // (ng: uniform)
        };
        // the region of cell `e`, fetched with the cross sections of its step (0 without the flag)
        [[maybe_unused]] auto load_region = [&](const int32_t e) -> int32_t {
            if constexpr (IFACE) return a.if_region[e];
            else return 0;
        };
        // step t visits row r(t): 0, 1, ... forward; maxcnt-1, ..., 0 backward (demo/makie.jl:103: "the segments are stored in
        // reverse order for backward tracks"), all lanes in lockstep — a lane is active while r(t) < its count.  Steps beyond
        // the end are clamped to the last one (prefetches only).
        auto row_of = [&](const int t) -> int {
            const int tc = t < maxcnt ? t : maxcnt - 1;
            return dir ? maxcnt - 1 - tc : tc;
        };
        // cross sections of GP groups of cell `e` (a padded group repeats the last real one; its result is never used)
        auto load_xs = [&](const int32_t e, double (&st)[GP], double (&qs)[GP], double (&h)[NH]) {
            const RT_G double *x = a.xs + ((int64_t)e * a.G + a.g0) * 2;
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                const int gi = g < ng ? g : ng - 1;
                st[g] = x[2 * gi]; qs[g] = x[2 * gi + 1];
            }
            if constexpr (AN) {
                const RT_G double *x1 = a.xs1 + ((int64_t)e * a.G + a.g0) * 2;
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const int gi = g < ng ? g : ng - 1;
                    h[2 * g] = x1[2 * gi]; h[2 * g + 1] = x1[2 * gi + 1];
                }
            }
            if constexpr (LS) { h[2 * GP] = a.cen[(int64_t)e * 2]; h[2 * GP + 1] = a.cen[(int64_t)e * 2 + 1]; }
        };
        ExpPoly poly = exp_poly();  // (in vector registers: see one_minus_exp_neg)
#pragma unroll
        for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(poly.c[i]));
        // one segment: attenuation and tally for the GP groups of this pass.  A lane beyond its track's end evaluates a segment
        // of length 0: τ = 0, 1 − e^{−0} = 0 exactly, Δ = ±0 — its ψ keeps its bits, and one select does for all groups.
        // (dsl: the row's slot in DSweep::delta, read by the REPRO instantiations only)
        auto segment = [&](const int32_t e, const double ell_row, const bool act, const double (&st)[GP], const double (&qs0)[GP],
                           const double (&h)[NH], [[maybe_unused]] const int64_t dsl, [[maybe_unused]] const int32_t rg = 0) {
            const double ell = act ? ell_row : 0.0;
            // IFACE: ψ as it stands between the previous record and this one crosses into region rg (rare and divergent; ahead of the
            // arithmetic and far from the fold).  An inactive lane — beyond its track's end, or a backward lane before its track's first
            // row — neither tallies nor moves its register.
            if constexpr (IFACE) {
                if (act) {
                    if (rg != rprev) iface_add(rprev, rg);
                    rprev = rg;
                }
            }
            double wd[NT * GP], tau[GP], qs[GP];
            bool thin = true;
            // LS: the midpoint relative to the cell's centroid; s moves on by ℓ (0 for a lane beyond its track's end)
            double xi = 0.0, eta = 0.0;
            if constexpr (LS) {
                const double sm = __builtin_fma(0.5, ell, srun);
                xi = __builtin_fma(dcs, sm, ex - h[2 * GP]);
                eta = __builtin_fma(dsn, sm, ey - h[2 * GP + 1]);
                srun += ell;
            }
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                tau[g] = st[g] * ell;
                thin = thin && tau[g] < kThinTau;
                if constexpr (P1) qs[g] = __builtin_fma(dsn, h[2 * g + 1], __builtin_fma(dcs, h[2 * g], qs0[g]));
                else if constexpr (LS) qs[g] = __builtin_fma(st[g], __builtin_fma(eta, h[2 * g + 1], xi * h[2 * g]), qs0[g]);  // r_m
                else qs[g] = qs0[g];
            }
            // LS: one component from F1 = 1 − e^{−τ} and hF2 = F2/2 (see the head of the kernel)
            [[maybe_unused]] auto ls_component = [&](const int g, const double F1, const double hF2) {
                const double rho = __builtin_fma(dsn, h[2 * g + 1], dcs * h[2 * g]);  // ρ / Σ_c
                const double am = psi[g] - qs[g];
                // (−ρ hF2 as an fma onto +0 rather than a negated product — the same value, and never −0: at τ = 0 both terms of d are
                //  zeros, d is +0 whatever the signs of ψ − r_m and ρ, and ψ − d keeps ψ's bits, those of ψ = −0 included)
                const double d = __builtin_fma(am, F1, __builtin_fma(-rho, hF2, 0.0));
                const double Hs = __builtin_fma(rho, __builtin_fma(0.5, tau[g], 1.0), am) * hF2;  // Σ_c H
                psi[g] = psi[g] - d;
                wd[g] = w * d;
                const double ws = wd[g] * st[g];
                wd[GP + 2 * g] = __builtin_fma(xi, ws, -(wcs * Hs));
                wd[GP + 2 * g + 1] = __builtin_fma(eta, ws, -(wsn * Hs));
            };
            // −expm1(−τ) to within an ulp (rt_device.hpp): where every lane's segment is optically thin in every group of the pass —
            // a wave-uniform branch — by the series alone (10 instructions per group instead of 24)
            // (The choice is per WAVE-row: a segment takes the series when the other 63 lanes' segments are thin too, else the general
            //  form — the two agree to 2 ulp, so ψ_out is NOT bitwise invariant across march orders, sort modes or shardings of the
            //  same problem; the tests compare at 1e-12.  "sweep_debug" 4 = the general form everywhere: the reproducible mode.)
            if constexpr (LS) {
                if (__ballot(!thin) == 0 && !(a.debug & 4)) {
#pragma unroll
                    for (int g = 0; g < GP; ++g) ls_component(g, one_minus_exp_neg_thin(tau[g], poly), 0.5 * ls_f2_thin(tau[g]));
                } else {
#pragma unroll
                    for (int g = 0; g < GP; ++g) {
                        double E;
                        const double F1 = one_minus_exp_neg_both(tau[g], E, poly);
                        ls_component(g, F1, 0.5 * ls_f2(tau[g], E));
                    }
                }
            } else if (__ballot(!thin) == 0 && !(a.debug & 4)) {
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const double d = (psi[g] - qs[g]) * one_minus_exp_neg_thin(tau[g], poly);
                    psi[g] = psi[g] - d;
                    if constexpr (VOID) {  // (Σt = 0: d is a zero and ψ kept its bits — the track length ψ ℓ in Δψ's place)
                        const double tv = st[g] == 0.0 ? psi[g] * ell : d;
                        wd[g] = w * tv;
                        if constexpr (P1) { wd[GP + 2 * g] = wcs * tv; wd[GP + 2 * g + 1] = wsn * tv; }
                    } else {
                        wd[g] = w * d;
                        if constexpr (P1) { wd[GP + 2 * g] = wcs * d; wd[GP + 2 * g + 1] = wsn * d; }
                    }
                }
            } else {
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const double d = (psi[g] - qs[g]) * one_minus_exp_neg(tau[g], poly);
                    psi[g] = psi[g] - d;
                    if constexpr (VOID) {
                        const double tv = st[g] == 0.0 ? psi[g] * ell : d;
                        wd[g] = w * tv;
                        if constexpr (P1) { wd[GP + 2 * g] = wcs * tv; wd[GP + 2 * g + 1] = wsn * tv; }
                    } else {
                        wd[g] = w * d;
                        if constexpr (P1) { wd[GP + 2 * g] = wcs * d; wd[GP + 2 * g + 1] = wsn * d; }
                    }
                }
            }
            // REPRO: no fold and no add — every active lane stores its NT·GP values at its (row slot, direction) of the delta buffer, and
            // k_sweep_reduce sums them per cell after the pass
            if constexpr (REPRO) {
                if (act) {
                    RT_G double *dst = a.delta + ((int64_t)dir * a.dslots + dsl) * (NT * GP);
#pragma unroll
                    for (int g = 0; g < NT * GP; ++g) dst[g] = wd[g];
                }
                return;
            }
            // Neighbouring lanes are neighbouring parallel tracks: at the same row most of them are in the same cell, and
            // atomics of one wave instruction to one address are served one lane at a time (measured at C3: the tallies were
            // 0.21 of the sweep's 0.62 ms).  Lanes of an aligned pair, then quad, with equal cells are therefore summed first —
            // two DPP row shifts, no LDS traffic — and only the lanes left over add to the tally.  The sweep is bound by
            // instruction issue, so folding further costs more than the atomics it saves: over 2 / 4 / 8 / 16 lanes the
            // sweep took 0.440 / 0.438 / 0.466 / 0.494 ms (0.414 without any tally).
            bool mine = act;
            if (!(a.debug & 2)) {
                const int32_t key = act ? e : -1 - lane;  // (an inactive lane matches nobody)
                // lane l with (l mod 2n) == 0 takes over lane l + n (row_shl:n reads lane l + n of the 16-lane row)
                auto fold = [&]<int NSH>() {
                    // (bound_ctrl: a lane whose source lies outside its row reads 0 and no `old` value has to be moved in first;
                    //  the lanes that use what they read — `take`, `given` — never read across a row's end)
                    const int32_t key_up = __builtin_amdgcn_update_dpp(0, key, 0x100 + NSH, 0xf, 0xf, true);
                    const int32_t key_dn = __builtin_amdgcn_update_dpp(0, key, 0x110 + NSH, 0xf, 0xf, true);
                    const bool take = ((lane & (2 * NSH - 1)) == 0) && key_up == key;
                    const bool given = ((lane & (2 * NSH - 1)) == NSH) && key_dn == key;
#pragma unroll
                    for (int g = 0; g < NT * GP; ++g) {
                        const uint64_t bits = __builtin_bit_cast(uint64_t, wd[g]);
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)bits, 0x100 + NSH, 0xf, 0xf, true);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)(bits >> 32), 0x100 + NSH, 0xf, 0xf, true);
                        const double up = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
                        wd[g] = __builtin_fma(up, take ? 1.0 : 0.0, wd[g]);  // (one instruction; the values are finite)
                    }
                    mine = mine && !given;
                };
                fold.template operator()<1>(); fold.template operator()<2>();
            }
            if (mine && !(a.debug & 1)) {
#pragma unroll
                for (int g = 0; g < GP; ++g)
                    if (g < ng) {  // (uniform)
                        if (LDS) atomicAdd(&hist[e * (NT * GP) + g], wd[g]);
                        else unsafeAtomicAdd((double *)&a.phi[(int64_t)e * a.G + a.g0 + g], wd[g]);
                        if constexpr (AN) {
                            if (LDS) {
                                atomicAdd(&hist[e * (NT * GP) + GP + 2 * g], wd[GP + 2 * g]);
                                atomicAdd(&hist[e * (NT * GP) + GP + 2 * g + 1], wd[GP + 2 * g + 1]);
                            } else {
                                RT_G double *cu = a.cur + ((int64_t)e * a.G + a.g0 + g) * 2;
                                unsafeAtomicAdd((double *)cu, wd[GP + 2 * g]);
                                unsafeAtomicAdd((double *)(cu + 1), wd[GP + 2 * g + 1]);
                            }
                        }
                    }
            }
        };
        if (maxcnt > 0) {
            if (STAGED) {
                // the wave's chunk ids: lane j holds chunks j, j + 64, ... (kMaxChunks = 313: five registers cover MAX_ITER rows)
                const RT_G int32_t *ctab = a.stg.ctab + mw * kMaxChunks;
                const int nchunks = (maxcnt + kChunkRows - 1) >> kChunkLog2;
                int32_t cv[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) cv[k] = (k * 64 + lane < nchunks) ? ctab[k * 64 + lane] : 0;
                // (v_readlane reads a lane whether or not it is active: call this in wave-uniform control flow only — inside a
                //  divergent branch the selected register of an inactive holder lane is stale)
                auto chunk_of = [&](const int r) -> int32_t {
                    const int j = r >> kChunkLog2;
                    const int32_t v = j < 64 ? cv[0] : (j < 128 ? cv[1] : (j < 192 ? cv[2] : (j < 256 ? cv[3] : cv[4])));
                    return __builtin_amdgcn_readlane(v, j & 63);
                };
                struct Row { double qx, qy; int32_t el; };
                // the chunk id of a row is looked up only when the row stream enters another 32-row chunk (two streams: the row
                // being evaluated and the one being prefetched); both lookups stay in scalar registers
                int cj0 = -1, cj2 = -1;
                int32_t cid0 = 0, cid2 = 0;
                auto slot_cached = [&](const int r, int &cj, int32_t &cid) -> int64_t {
                    const int j = r >> kChunkLog2;
                    if (j != cj) { cj = j; cid = chunk_of(r); }  // (uniform)
                    return stage_slot(cid, r & (kChunkRows - 1), lane);
                };
                auto slot_of = [&](const int r) -> int64_t { return stage_slot(chunk_of(r), r & (kChunkRows - 1), lane); };
                auto load_row = [&](const int r) -> Row {
                    const int64_t sl = slot_of(r);
                    return Row{a.stg.qx[sl], a.stg.qy[sl], a.stg.element[sl]};
                };
                auto cell_of = [&](const Row &R, const int r) -> int32_t { return r < cnt ? (R.el < 0 ? -R.el : R.el) - 1 : 0; };
                // One step: Ra holds row r(t), Rb row r(t + 1) and Rc — until this step's prefetch replaces it — row r(t − 1).  The
                // loop is unrolled three times with the roles rotated, so that no row register is moved from one stage of the
                // pipeline to the next; steps t >= maxcnt of the last round do nothing (act is false, their loads are clamped).
                // Measured at C3, 7 groups, same box: rotating by moves 0.373 ms, three steps per round 0.358, six (the cross
                // sections' two stages rotated as well; 32 scalar registers spilled) 0.366; one copy of the loop per direction
                // (forward and backward waves of a CU then run different code) 0.396.
                if constexpr (!ELLROWS) {
                    const int DIR = dir;
                    auto row_d = row_of;
                    Row R0 = load_row(row_d(0)), R1 = load_row(row_d(1)), R2{0.0, 0.0, 0};
                    double stA[GP], qsA[GP], stB[GP], qsB[GP], hA[NH], hB[NH];
                    load_xs(cell_of(R0, row_d(0)), stA, qsA, hA);
                    auto step = [&](const int t, const Row &Ra, const Row &Rb, Row &Rc, const double (&st0)[GP], const double (&qs0)[GP],
                                    const double (&h0)[NH], double (&st1)[GP], double (&qs1)[GP], double (&h1)[NH]) {
                        const int r = row_d(t);
                        const bool act = r < cnt && t < maxcnt;
                        // entry point: the previous record's exit point — forward the row before, backward the NEXT step's row — or,
                        // for marked records (cell < 0: first record of a track, records of the generic step), the staged one
                        double dx = (DIR ? Rb.qx : Rc.qx) - Ra.qx, dy = (DIR ? Rb.qy : Rc.qy) - Ra.qy;
                        const int64_t sl0 = slot_cached(r, cj0, cid0);  // (outside the branch: see chunk_of)
                        double px = 0.0, py = 0.0;
                        const bool marked = act && Ra.el < 0;
                        if (marked) { px = a.stg.px[sl0]; py = a.stg.py[sl0]; }
                        const int64_t sl2 = slot_cached(row_d(t + 2), cj2, cid2);
                        Rc = Row{a.stg.qx[sl2], a.stg.qy[sl2], a.stg.element[sl2]};
                        load_xs(cell_of(Rb, row_d(t + 1)), st1, qs1, h1);
                        if (marked) { dx = px - Ra.qx; dy = py - Ra.qy; }
                        const double ell = norm2(dx, dy);  // Segment ctor, src/segment.jl:31-33 (as k_compact3)
                        if (a.ell_rows != nullptr && !DIR && act) a.ell_rows[sl0] = ell;  // (uniform && uniform && lane: for the ELLROWS passes)
                        segment(cell_of(Ra, r), ell, act, st0, qs0, h0, sl0);
                    };
                    for (int t = 0; t < maxcnt; t += 3) {
                        step(t, R0, R1, R2, stA, qsA, hA, stB, qsB, hB);
                        step(t + 1, R1, R2, R0, stB, qsB, hB, stA, qsA, hA);
                        step(t + 2, R2, R0, R1, stA, qsA, hA, stB, qsB, hB);
#pragma unroll
                        for (int g = 0; g < GP; ++g) { stA[g] = stB[g]; qsA[g] = qsB[g]; }
                        if constexpr (AN)
#pragma unroll
                            for (int g = 0; g < NH; ++g) hA[g] = hB[g];
                    }
                }
                if constexpr (ELLROWS) {
                    // the same pipeline over (ℓ, cell) rows — ℓ as an earlier pass over these staging rows left it: 12 B per row instead
                    // of 20, no square root, no entry point to pick
                    struct LRow { double ell; int32_t el; };
                    auto load_lrow = [&](const int64_t sl) -> LRow { return LRow{a.ell_rows[sl], a.stg.element[sl]}; };
                    auto lcell = [&](const LRow &R, const int r) -> int32_t { return r < cnt ? (R.el < 0 ? -R.el : R.el) - 1 : 0; };
                    LRow L0 = load_lrow(slot_of(row_of(0))), L1 = load_lrow(slot_of(row_of(1))), L2{0.0, 0};
                    double stA[GP], qsA[GP], stB[GP], qsB[GP], hA[NH], hB[NH];
                    load_xs(lcell(L0, row_of(0)), stA, qsA, hA);
                    // (IFACE: the cells' regions travel with the cross sections' two stages)
                    [[maybe_unused]] int32_t rgA = load_region(lcell(L0, row_of(0))), rgB = 0;
                    auto lstep = [&](const int t, const LRow &Ra, const LRow &Rb, LRow &Rc, const double (&st0)[GP], const double (&qs0)[GP],
                                     const double (&h0)[NH], double (&st1)[GP], double (&qs1)[GP], double (&h1)[NH],
                                     [[maybe_unused]] const int32_t rg0, [[maybe_unused]] int32_t &rg1) {
                        const int r = row_of(t);
                        const bool act = r < cnt && t < maxcnt;
                        int64_t sl0 = 0;
                        if constexpr (REPRO) sl0 = slot_cached(r, cj0, cid0);  // (the slot of the row being evaluated: uniform lookup, see chunk_of)
                        Rc = load_lrow(slot_cached(row_of(t + 2), cj2, cid2));
                        load_xs(lcell(Rb, row_of(t + 1)), st1, qs1, h1);
                        if constexpr (IFACE) rg1 = load_region(lcell(Rb, row_of(t + 1)));
                        segment(lcell(Ra, r), Ra.ell, act, st0, qs0, h0, sl0, rg0);
                    };
                    for (int t = 0; t < maxcnt; t += 3) {
                        lstep(t, L0, L1, L2, stA, qsA, hA, stB, qsB, hB, rgA, rgB);
                        lstep(t + 1, L1, L2, L0, stB, qsB, hB, stA, qsA, hA, rgB, rgA);
                        lstep(t + 2, L2, L0, L1, stA, qsA, hA, stB, qsB, hB, rgA, rgB);
                        if constexpr (IFACE) rgA = rgB;
#pragma unroll
                        for (int g = 0; g < GP; ++g) { stA[g] = stB[g]; qsA[g] = qsB[g]; }
                        if constexpr (AN)
#pragma unroll
                            for (int g = 0; g < NH; ++g) hA[g] = hB[g];
                    }
                }
            } else {
                struct Rec { double ell; int32_t el; };
                auto load_rec = [&](const int r) -> Rec {
                    const int rc = r < cnt ? r : (cnt > 0 ? cnt - 1 : 0);  // (a lane's own records only; masked where r >= cnt)
                    if (cnt == 0) return Rec{0.0, 1};                      // (a track without records: offsets[u] may equal the total)
                    return Rec{a.ell[off + rc], a.element[off + rc]};
                };
                auto cell_of = [&](const Rec &R, const int r) -> int32_t { return r < cnt ? R.el - 1 : 0; };
                Rec R0 = load_rec(row_of(0)), R1 = load_rec(row_of(1));
                double st0[GP], qs0[GP], h0[NH];
                load_xs(cell_of(R0, row_of(0)), st0, qs0, h0);
                for (int t = 0; t < maxcnt; ++t) {
                    const int r = row_of(t);
                    const Rec R2 = load_rec(row_of(t + 2));
                    double st1[GP], qs1[GP], h1[NH];
                    load_xs(cell_of(R1, row_of(t + 1)), st1, qs1, h1);
                    segment(cell_of(R0, r), R0.ell, r < cnt, st0, qs0, h0, off + r);
                    R0 = R1; R1 = R2;
#pragma unroll
                    for (int g = 0; g < GP; ++g) { st0[g] = st1[g]; qs0[g] = qs1[g]; }
                    if constexpr (AN)
#pragma unroll
                        for (int g = 0; g < NH; ++g) h0[g] = h1[g];
                }
            }
        }
        if (have)
#pragma unroll
            for (int g = 0; g < GP; ++g)
                if (g < ng) a.psi_out[pbase + g] = psi[g];
        // IFACE: ψ_out leaves the last record's region (a track without records tallies nothing)
        if constexpr (IFACE)
            if (have && cnt > 0) iface_add(rprev, a.if_R);
    }
    if (LDS || IFACE) __syncthreads();
    if constexpr (IFACE)
        for (int c = threadIdx.x; c < ntab; c += blockDim.x) {
            const double v = itab[c];
            const int pair = c / GP, g = c - pair * GP;
            if (v != 0.0 && g < a.ng) unsafeAtomicAdd((double *)&a.if_S[(int64_t)pair * a.G + a.g0 + g], v);
        }
    if (LDS) {
        for (int c = threadIdx.x; c < a.n_cells * (NT * GP); c += blockDim.x) {
            const double v = hist[c];
            const int cell = c / (NT * GP), i = c - cell * (NT * GP);
            if (!AN || i < GP) {
                if (v != 0.0 && i < a.ng) unsafeAtomicAdd((double *)&a.phi[(int64_t)cell * a.G + a.g0 + i], v);
            } else {
                const int g = (i - GP) >> 1;
                if (v != 0.0 && g < a.ng) unsafeAtomicAdd((double *)&a.cur[((int64_t)cell * a.G + a.g0 + g) * 2 + ((i - GP) & 1)], v);
            }
        }
    }
