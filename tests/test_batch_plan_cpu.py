"""The continuous batch driver's planner (csrc/vox_batch_plan.cpp: step_costs, plan_slots, the retire-slack schedule) against an independent restatement written here.
Host arithmetic only: vox_debug_step_costs / vox_debug_plan_slots take no context and touch no device, so nothing in this file needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRE_SLACK = 12


def shipped_tables():
    """kStepMs / kStepMsEng as csrc/vox_api.cpp ships them (read from the source, so a re-measured table is followed), each also with the four-group entry the driver
    overrides on a GPU of its own (two two-group wide chains: 2.95 ms)."""
    src = open(os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "csrc", "vox_api.cpp")).read()
    tabs = []
    for name in ("kStepMs", "kStepMsEng"):
        m = re.search(r"static const double %s\[9\] = \{([^}]*)\}" % name, src)
        t = [float(v) for v in m.group(1).split(",")]
        assert len(t) == 9 and t[0] == 0.0 and all(b >= a for a, b in zip(t, t[1:])), (name, t)
        tabs.append(t); tabs.append(t[:4] + [2.95] + t[5:])
    return tabs


def ref_step_costs(base, meas, calib, shared):
    ratio, nr = 0.0, 0
    for g in range(1, 9):
        if calib and meas[g] > 0.0:
            ratio += meas[g] / base[g]; nr += 1
    ratio = min(4.0, max(0.25, ratio / nr)) if nr else 1.0
    out = [0.0] * 9
    for g in range(1, 9):
        common = base[g] * ratio
        v = common * min(1.15, max(0.85, meas[g] / common)) if (calib and not shared and meas[g] > 0.0) else common
        out[g] = max(v, out[g - 1])
    return out


def ref_plan(steps, force_G, max_groups, step_ms):
    """LPT: jobs stably sorted by steps descending, each onto the least loaded of 16 G slots (first wins a tie), slots stably ordered by load descending, a group's
    steps the maximum of its 16 slots, cost the staircase sum; of all G the cheapest, the larger on a tie; then the 12-step retire slack."""
    n = len(steps)
    jobs = sorted(range(n), key=lambda i: -steps[i])
    g_max = max(1, min(max_groups, (n + 15) // 16))
    best = None
    for G in range(1, g_max + 1):
        if force_G > 0 and G != min(force_G, g_max):
            continue
        Sl = 16 * G; load = [0] * Sl; q = [[] for _ in range(Sl)]
        for j in jobs:
            b = min(range(Sl), key=lambda s: (load[s], s))
            load[b] += steps[j]; q[b].append(j)
        order = sorted(range(Sl), key=lambda s: -load[s])
        steps_g = [max(load[s] for s in order[16 * k:16 * k + 16]) for k in range(G)]
        cost = 0.0
        for k in range(G):
            cost += float(steps_g[k] - (steps_g[k + 1] if k + 1 < G else 0)) * step_ms[k + 1]
        if best is None or cost <= best["cost"]:
            best = dict(G=G, queue=[q[s] for s in order], steps_g=steps_g, cost=cost)
    run_g = list(best["steps_g"])
    for gi in range(1, best["G"]):
        if run_g[gi - 1] - best["steps_g"][gi] < RETIRE_SLACK:
            run_g[gi] = run_g[gi - 1]
    best["run_g"] = run_g
    return best


def lib_step_costs(pkg, base, meas, calib, shared):
    b = (C.c_double * 9)(*base); m = (C.c_double * 9)(*meas); out = (C.c_double * 9)()
    pkg._lib.check(pkg.lib().vox_debug_step_costs(b, m, int(calib), int(shared), out))
    return list(out)


def lib_plan(pkg, steps, force_G, max_groups, step_ms):
    n = len(steps)
    st = (C.c_int32 * max(n, 1))(*steps); ms = (C.c_double * 9)(*step_ms)
    G = C.c_int32(-1); slot = (C.c_int32 * max(n, 1))(*([-1] * max(n, 1))); qpos = (C.c_int32 * max(n, 1))(*([-1] * max(n, 1)))
    sg = (C.c_int32 * 8)(*([-1] * 8)); rg = (C.c_int32 * 8)(*([-1] * 8)); cost = C.c_double(-1.0)
    pkg._lib.check(pkg.lib().vox_debug_plan_slots(st, n, force_G, max_groups, ms, C.byref(G), slot, qpos, sg, rg, C.byref(cost)))
    return dict(G=G.value, slot=list(slot)[:n], qpos=list(qpos)[:n], steps_g=list(sg), run_g=list(rg), cost=cost.value)


def check_plan(pkg, steps, force_G, max_groups, step_ms):
    got = lib_plan(pkg, steps, force_G, max_groups, step_ms); ref = ref_plan(steps, force_G, max_groups, step_ms)
    G = got["G"]; tag = (len(steps), force_G, max_groups)
    assert G == ref["G"], tag
    assert 1 <= G <= max_groups and (force_G == 0 or G == min(force_G, max(1, min(max_groups, (len(steps) + 15) // 16)))), tag
    # every job exactly once: a slot of the plan, a queue position no other job of that slot has, the positions of a slot dense from 0
    queue = [[] for _ in range(16 * G)]
    for j, (s, k) in enumerate(zip(got["slot"], got["qpos"])):
        assert 0 <= s < 16 * G and k >= 0, (tag, j, s, k)
        queue[s].append((k, j))
    for s in range(16 * G):
        queue[s].sort()
        assert [k for k, _ in queue[s]] == list(range(len(queue[s]))), (tag, s)
    assert [[j for _, j in q] for q in queue] == ref["queue"], tag
    assert sum(len(q) for q in queue) == len(steps)
    sg, rg = got["steps_g"], got["run_g"]
    assert sg[:G] == ref["steps_g"] and rg[:G] == ref["run_g"] and sg[G:] == [0] * (8 - G) and rg[G:] == [0] * (8 - G), tag
    assert got["cost"] == ref["cost"], tag
    # properties, from the plan alone
    load = [sum(steps[j] for _, j in q) for q in queue]
    assert all(a >= b for a, b in zip(load, load[1:])), tag                                   # slots ordered by load ...
    assert sg[:G] == [max(load[16 * k:16 * k + 16]) for k in range(G)], tag                  # ... a group's steps its slots' maximum ...
    assert all(a >= b for a, b in zip(sg[:G], sg[1:G])), tag                                 # ... so the groups retire last to first
    assert all(a >= b for a, b in zip(rg[:G], rg[1:G])) and all(r >= s for r, s in zip(rg[:G], sg[:G])) and (rg[0] == sg[0]), tag
    for gi in range(1, G):
        assert rg[gi] == (rg[gi - 1] if rg[gi - 1] - sg[gi] < RETIRE_SLACK else sg[gi]), (tag, gi)
    return got


def corpus_steps(pkg, n=647):
    cfg = pkg.PadConfig.voxtral()
    durs = pkg.shard.fleurs_like_durations(n, seed=7)
    steps = [cfg.padded_len(int(round(d * 16000))) // 2560 - 39 for d in durs]
    assert min(steps) >= 1
    return durs, steps


def workloads(pkg):
    durs, steps = corpus_steps(pkg)
    out = [("corpus", steps)]
    for r, part in enumerate(pkg.shard.lpt_partition(durs, 8)):
        out.append((f"share{r}", [steps[i] for i in part]))
    out += [("seventeen", steps[:17]), ("one", steps[:1]), ("none", []), ("equal32", [100] * 32), ("equal81", [57] * 81), ("equal128", [9] * 128)]
    return out


def test_step_costs_match_restatement(pkg):
    rng = np.random.default_rng(11)
    for base in shipped_tables():
        zero = [0.0] * 9
        for shared in (0, 1):
            assert lib_step_costs(pkg, base, zero, 1, shared) == base          # nothing measured yet: the table
            meas_all = [0.0] + [b * 1.3 for b in base[1:]]
            assert lib_step_costs(pkg, base, meas_all, 0, shared) == base      # calibration off: the table
        cases = [zero, [0.0, 2.0] + [0.0] * 7, [0.0, 0.1] + [0.0] * 7, [0.0, 40.0] + [0.0] * 7,      # one form seen; ratio clamped at 0.25 and at 4
                 [0.0, 2.0, 2.3, 5.35, 4.18, 0.0, 0.0, 0.0, 0.0],                                      # a three-group step measured above four groups
                 [0.0] + [b * 1.5 for b in base[1:]], [0.0] + [b * (1.5 if g % 2 else 0.7) for g, b in enumerate(base[1:], 1)]]
        cases += [[0.0] + [float(v) if rng.random() < 0.6 else 0.0 for v in rng.uniform(0.2, 12.0, 8)] for _ in range(40)]
        for meas in cases:
            for calib in (0, 1):
                for shared in (0, 1):
                    got = lib_step_costs(pkg, base, meas, calib, shared)
                    assert got == ref_step_costs(base, meas, calib, shared), (base, meas, calib, shared)
                    assert got[0] == 0.0 and all(b >= a for a, b in zip(got, got[1:])), (meas, got)      # more groups never cost less
                    if not calib:
                        assert got == base


def test_plan_slots_matches_restatement_on_corpus_and_shares(pkg):
    for base in shipped_tables():
        for name, steps in workloads(pkg):
            for max_groups in (4, 8):
                got = check_plan(pkg, steps, 0, max_groups, base)
                if name == "none":
                    assert got["G"] == 1 and got["steps_g"] == [0] * 8 and got["cost"] == 0.0
                if name == "one":
                    assert got["G"] == 1 and got["slot"] == [0] and got["qpos"] == [0] and got["steps_g"][0] == steps[0]


def test_plan_slots_every_forced_group_count(pkg):
    base = shipped_tables()[0]
    for name, steps in workloads(pkg):
        for max_groups in (4, 8):
            for force_G in range(1, 9):
                check_plan(pkg, steps, force_G, max_groups, base)


def test_plan_slots_calibrated_costs_and_ties(pkg):
    """Plans priced with calibrated costs (the planner's real input on a warm context), and the tie rule: of two group counts that cost the same, the larger."""
    durs, steps = corpus_steps(pkg)
    share = [steps[i] for i in pkg.shard.lpt_partition(durs, 8)[0]]
    for base in shipped_tables():
        for meas in ([0.0, 2.0, 2.3, 5.35, 4.18, 0.0, 0.0, 0.0, 0.0], [0.0] + [b * 0.8 for b in base[1:]]):
            for shared in (0, 1):
                cost = lib_step_costs(pkg, base, meas, 1, shared)
                for w in (steps, share):
                    check_plan(pkg, w, 0, 8, cost)
    tie = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]      # 32 equal jobs: one group runs 2 L steps at 1.0, two groups L steps at 2.0 -- the same cost
    got = check_plan(pkg, [100] * 32, 0, 8, tie)
    assert got["G"] == 2 and got["cost"] == 200.0
    got = check_plan(pkg, [50] * 128, 0, 8, tie)
    assert got["G"] == 8 and got["cost"] == 400.0
    assert check_plan(pkg, [50] * 128, 0, 4, tie)["G"] == 4


def test_plan_slots_retire_slack(pkg):
    """A group that would retire fewer than 12 steps before the next longer one runs on with it; 12 or more: it retires on its own."""
    flat = [0.0] + [1.0] * 8
    for gap, snapped in ((0, True), (1, True), (11, True), (12, False), (40, False)):
        steps = [100] * 16 + [100 - gap] * 16
        got = check_plan(pkg, steps, 2, 8, flat)
        assert got["steps_g"][:2] == [100, 100 - gap] and got["run_g"][:2] == [100, 100 if snapped else 100 - gap], gap
    got = check_plan(pkg, [100] * 16 + [95] * 16 + [90] * 16 + [60] * 16, 4, 4, flat)      # the slack chains on the RUN length of the group before
    assert got["run_g"][:4] == [100, 100, 100, 60]


def test_planner_exports_refuse_bad_arguments(pkg):
    L = pkg.lib(); ms = (C.c_double * 9)(*([0.0] + [1.0] * 8)); out = (C.c_double * 9)()
    assert L.vox_debug_step_costs(None, ms, 1, 0, out) == 1 and L.vox_debug_step_costs(ms, ms, 1, 0, None) == 1
    st = (C.c_int32 * 2)(5, 0); G = C.c_int32(); a = (C.c_int32 * 2)(); b = (C.c_int32 * 2)(); sg = (C.c_int32 * 8)(); rg = (C.c_int32 * 8)(); cost = C.c_double()
    assert L.vox_debug_plan_slots(st, 2, 0, 4, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 1      # a job of 0 steps
    assert L.vox_debug_plan_slots(st, 1, 9, 4, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 1 and L.vox_debug_plan_slots(st, 1, 0, 9, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 1
    assert L.vox_debug_plan_slots(st, 1, 0, 0, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 1 and L.vox_debug_plan_slots(st, -1, 0, 4, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 1
    assert L.vox_debug_plan_slots(st, 1, 0, 4, ms, C.byref(G), a, b, sg, rg, C.byref(cost)) == 0 and G.value == 1
