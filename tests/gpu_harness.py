"""Drive the HIP env (through the C ABI) and the CPU oracle over the same multi-episode action
tables. Used by the gpu tests and __graft_entry__.smoke()."""
import numpy as np

from ast_sac_amd import shipsim_abi as abi


def make_tables(n_envs, n_episodes, seed=20251015, special=True):
    """Per env: list of episodes, each 9 normalized actions. The first envs replay the golden
    fixture tables (zero actions, seeded tables, all +1 / all -1 -> sampling failures)."""
    tables = []
    fixed = [np.zeros(9, np.float32), np.ones(9, np.float32), -np.ones(9, np.float32)]
    for i in range(n_envs):
        rng = np.random.Generator(np.random.PCG64(seed + i))
        eps = [rng.uniform(-1, 1, 9).astype(np.float32) for _ in range(n_episodes)]
        if special and i < len(fixed):
            eps[0] = fixed[i]
        tables.append(eps)
    return tables


def run_oracle(cfg, tables):
    import oracle_ffi as O
    out = []
    for eps in tables:
        env = O.OracleEnv(cfg)
        rec = []
        for table in eps:
            o0 = env.reset()
            decs = []
            for a_norm in table:
                a = abi.normalized_to_scoping(a_norm)
                o, r, d, bits, ticks = env.step(a)
                decs.append((o, r, d, bits, ticks))
                if d:
                    break
            rec.append((o0, decs))
        ships = np.array([env.ship_state(s) for s in range(cfg.n_ships)])
        out.append((rec, ships, env.env_state()))
    return out


def run_gpu(cfg, tables, device="cuda", max_ticks=0):
    """Replay `tables` through ShipSim. With max_ticks > 0 decisions are sliced: every call runs at
    most max_ticks ticks per env and the harness keeps calling until each decision completes."""
    import torch
    from ast_sac_amd.shipsim import ShipSim
    n = len(tables)
    sim = ShipSim(cfg, n, device=device)
    o0 = sim.reset().cpu().numpy()
    ep = np.zeros(n, int)
    dec = np.zeros(n, int)
    acc_ticks = np.zeros(n, int)
    rec = [[(o0[i].copy(), [])] for i in range(n)]
    n_eps = np.array([len(t) for t in tables])
    calls = 0
    while True:
        active = ep < n_eps
        if not active.any():
            break
        acts = np.zeros(n, np.float32)
        for i in np.nonzero(active)[0]:
            acts[i] = abi.normalized_to_scoping(tables[i][ep[i]][dec[i]])
        out = sim.step(torch.from_numpy(acts), active=torch.from_numpy(active.astype(np.uint8)), max_ticks=max_ticks)
        o = out["obs"].cpu().numpy()
        r = out["reward"].cpu().numpy()
        d = out["done"].cpu().numpy().astype(bool)
        b = out["events"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        t = out["ticks"].cpu().numpy()
        rd = out["ready"].cpu().numpy().astype(bool)
        calls += 1
        need_reset = np.zeros(n, bool)
        for i in np.nonzero(active)[0]:
            acc_ticks[i] += t[i]
            if not rd[i]:
                continue
            rec[i][-1][1].append((o[i].copy(), float(r[i]), bool(d[i]), int(b[i]), int(acc_ticks[i])))
            acc_ticks[i] = 0
            dec[i] += 1
            if d[i] or dec[i] >= len(tables[i][ep[i]]):
                ep[i] += 1
                dec[i] = 0
                if ep[i] < n_eps[i]:
                    need_reset[i] = True
        if need_reset.any():
            o0 = sim.reset(mask=torch.from_numpy(need_reset.astype(np.uint8))).cpu().numpy()
            for i in np.nonzero(need_reset)[0]:
                rec[i].append((o0[i].copy(), []))
    fields = {f: sim.get(f).cpu().numpy() for f in range(abi.N_SHIP_FIELDS)}
    env_fields = {f: sim.get(f).cpu().numpy() for f in (abi.E_SAMPLING_COUNT, abi.E_TRAVEL_DIST, abi.E_TRAVEL_TIME,
                                                         abi.E_ACC_REWARD, abi.E_N_BASE, abi.E_E_BASE,
                                                         abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST)}
    sim.close()
    return rec, fields, env_fields, calls


PERTURBATIONS = (0.0, 1e-15, -1e-15, 1e-13)


def run_oracle_variants(cfg, tables, eps_list=PERTURBATIONS):
    """The oracle from the exact initial condition and from initial conditions perturbed by a few
    ulps. The reference trajectories are not well-conditioned everywhere: the SBMPC cost is
    discontinuous (dist < d_safe_i, phi_o sectors) and saturated controllers switch near waypoint
    boundaries, so a libm ulp can move a trajectory onto the neighbouring branch. A device result
    is accepted when it matches (1e-5) an oracle run whose initial state is within 1e-13 relative
    of the configured one — the same envelope the oracle itself shows under such perturbations."""
    import copy
    out = []
    for eps in eps_list:
        c = copy.deepcopy(cfg)
        c.ship[0].initial_north_position_m *= 1 + eps
        c.ship[1].initial_east_position_m *= 1 - eps
        out.append(run_oracle(c, tables))
    return out


def _compare_env(g_eps, o_eps, rtol):
    from parity import rel_err
    worst = 0.0
    msgs = []
    if len(g_eps) != len(o_eps):
        return np.inf, [f"{len(g_eps)} episodes vs {len(o_eps)}"]
    for k, ((g0, gd), (o0, od)) in enumerate(zip(g_eps, o_eps)):
        if not np.array_equal(g0, o0):
            msgs.append(f"ep {k}: reset obs differ")
        if len(gd) != len(od):
            msgs.append(f"ep {k}: {len(gd)} decisions vs {len(od)}")
            worst = np.inf
            continue
        for j, (g, o) in enumerate(zip(gd, od)):
            if g[4] != o[4] or (g[3] & 0x7FFFF) != (o[3] & 0x7FFFF) or g[2] != o[2]:
                msgs.append(f"ep {k} dec {j}: ticks {g[4]}/{o[4]} bits {g[3]:x}/{o[3]:x} done {g[2]}/{o[2]}")
                worst = np.inf
                continue
            e = max(float(rel_err(g[0][None], o[0][None]).max()), float(abs(g[1] - o[1]) / (abs(o[1]) + 1e-6)))
            worst = max(worst, e)
            if e > rtol:
                msgs.append(f"ep {k} dec {j}: rel err {e:.3e}")
    return worst, msgs


def sensitive_envs(orcs, rtol=1e-5):
    """The envs in which some oracle variant's records (run_oracle_variants) differ from variant 0's, by the
    comparison a device result is held to (_compare_env): the envs the oracle itself shows to be ill-conditioned.
    Outside this set the oracle's variants agree, and a device result must match the unperturbed oracle."""
    return {i for i in range(len(orcs[0])) for orc in orcs[1:] if _compare_env(orc[i][0], orcs[0][i][0], rtol)[1]}


def check_sensitive(chosen, orcs, max_share=0.25):
    """The input condition and the per-env statement of the oracle-variant tests: at most max_share of the envs are
    sensitive (so the rest are pinned to the exact oracle), and every env matched only by a perturbed variant is
    one of them. Returns the sensitive set."""
    S = sensitive_envs(orcs)
    assert len(S) / len(chosen) <= max_share, (len(S), len(chosen))
    outside = sorted(set(np.nonzero(np.asarray(chosen) != 0)[0].tolist()) - S)
    assert not outside, f"envs off the unperturbed oracle although the oracle's variants agree: {outside[:20]}"
    return S


def compare(gpu_rec, orcs, rtol=1e-5):
    """gpu_rec vs a list of oracle variants (run_oracle_variants; a bare run_oracle result is
    accepted too). Returns (worst error over envs, mismatch messages, per-env chosen variant)."""
    if orcs and isinstance(orcs[0], tuple):
        orcs = [orcs]
    worst = 0.0
    msgs = []
    chosen = []
    for i, g_eps in enumerate(gpu_rec):
        best = None
        for v, orc in enumerate(orcs):
            w, m = _compare_env(g_eps, orc[i][0], rtol)
            if best is None or w < best[0]:
                best = (w, m, v)
            if not m:
                break
        worst = max(worst, best[0])
        chosen.append(best[2])
        msgs += [f"env {i}: {x}" for x in best[1]]
    return worst, msgs, np.array(chosen)
