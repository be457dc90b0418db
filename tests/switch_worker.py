"""Worker process for the launch paths behind an environment variable the library reads once per process (spawned by
test_switch_paths_cpu.py / test_switch_paths_gpu.py, one child per job, the variable set by the parent: switch_cases.JOBS).

    python switch_worker.py JOB OUT.json [--host]

Every job first PROVES its switch in force by a host query of the library whose value differs from a default process's; a job that
cannot prove it fails before it runs a case — it never silently tests the default path.  --host: the proof and the "listed under the
named branch" conditions only, no GPU.  Otherwise the job's cases run through the call helpers of test_exact_conv_gpu.py /
test_conv_x3_gpu.py and every comparison is of bits.  The result is a JSON object {job, proof, failures, calls, seconds}; failures are
the first_difference messages."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wt-pse-code_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import exact_cases as E           # noqa: E402
import switch_cases as S          # noqa: E402


def lib():
    from wtpse_hip import build
    from wtpse_hip.lib import lib as L
    build.build()                                   # no-op when up to date
    return L()


X3R_SETTINGS = {"x3": (1,), "x3r": (2, 0), "x3half": (1, 0), "x3sw": (1,)}
MT1_CASES = (("x3", (32, 64, 0, 64, 64, 64, 3)), ("x3r", (64, 32, 32, 128, 32, 16)))
HALF1_PROOF = (2, 32, 0, 64, 8, 8, 3)


def x3_job_cases(job):
    """-> [(table, index)] of a job that runs forward / data-gradient cases."""
    small = [(t, i) for t in ("x3", "x3r") for i, c in enumerate(E.TABLES[t]) if c[0] <= 3]
    sw64 = [("x3sw", i) for i, c in enumerate(E.X3_SMALL_WIDE_CASES) if c[3] % 64 == 0]
    if job == "mt2":
        return small + [("x3half", i) for i, c in enumerate(E.TABLES["x3half"]) if c[0] <= 3] + sw64
    if job == "mt1":
        return [(t, E.TABLES[t].index(c)) for t, c in MT1_CASES]
    if job == "half1":
        return small + sw64
    raise KeyError(job)


def x3_job_switches(job):
    return {"mt2": {"mt": 2}, "mt1": {"mt": 1}, "half1": {"half_min": 1}}[job]


def prove_x3(L, job):
    """The restated tiling under the job's switch == the library's size query on every launch of the job, in both directions and
    under every wtpse_x3r_enable setting its cases run; at least one of them differs from the default tiling; and the branches the
    job is about are taken.  -> (proof, problems)"""
    kw = x3_job_switches(job)
    changed, problems, seen = [], [], {"mt2_k1": False, "mt2_small_image": False, "mt2_ragged": False, "half_small_image": False, "half_ragged": False}
    for table, idx in x3_job_cases(job):
        B, C0, C1, Co, H, W, k = E.conv_shape(table, E.TABLES[table][idx])
        for x3r in X3R_SETTINGS[table]:
            was = L.query("wtpse_x3r_enable", x3r)
            try:
                for cout in (Co, C0 + C1):
                    t = E.x3_tiling(B, H, W, cout, k, x3r=x3r, **kw)
                    got = L.query("wtpse_conv_x3_stats_blocks", B, H, W, cout, k)
                    if got != t["tiles"]:
                        problems.append("%s %s cout %d x3r %d: the library has %d tiles, the restated tiling under %s has %d"
                                        % (table, (B, C0, C1, Co, H, W, k), cout, x3r, got, kw, t["tiles"]))
                    if t["tiles"] != E.x3_tiling(B, H, W, cout, k, x3r=x3r)["tiles"]:
                        changed.append((table, idx, cout, x3r))
                    ragged = H % t["TH"] != 0 or W % t["TW"] != 0
                    small_image = H < t["TH"] or W < t["TW"]
                    if t["mt"] == 2 and not t["half"]:
                        seen["mt2_k1"] |= k == 1
                        seen["mt2_small_image"] |= small_image
                        seen["mt2_ragged"] |= ragged and not small_image
                    if t["half"]:
                        seen["half_small_image"] |= small_image
                        seen["half_ragged"] |= ragged and not small_image
            finally:
                L.query("wtpse_x3r_enable", was)
    if not changed:
        problems.append("no launch of the job changes its tile count under the switch: it cannot be proved in force")
    if job == "mt2":
        need = ("mt2_k1", "mt2_small_image")
    elif job == "half1":
        need = ("half_small_image", "half_ragged")
        B, C0, C1, Co, H, W, k = HALF1_PROOF
        if E.x3_tiling(B, H, W, Co, k, **kw)["half"] != 1 or E.x3_tiling(B, H, W, Co, k)["half"] != 0:
            problems.append("%s must take the half tiles under the switch and not by default" % (HALF1_PROOF,))
    else:
        need = ()
        for table, idx in x3_job_cases(job):
            B, C0, C1, Co, H, W, k = E.conv_shape(table, E.TABLES[table][idx])
            if E.x3_tiling(B, H, W, Co, k, **kw)["mt"] == 2 and not E.x3_tiling(B, H, W, Co, k, **kw)["half"]:
                problems.append("%s still takes the 64-channel blocks on 256-pixel tiles" % ((B, C0, C1, Co, H, W, k),))
    problems += ["no case of the job reaches the branch '%s'" % n for n in need if not seen[n]]
    return {"launches_with_another_tile_count": len(changed), "branches": {k: v for k, v in seen.items() if k in need}}, problems


def prove_tw32(L):
    changed, problems = 0, []
    for fam in ("x3", "x3tw32"):
        for name in E.wgrad_cases(fam):
            B, C0, C1, Co, H, W = E.wgrad_cases(fam)[name][0]
            got = L.query("wtpse_wgrad_x3_ksplit", B, H, W, C0 + C1, Co)
            want = E.wgrad_x3_ksplit(B, H, W, C0 + C1, Co, tw32=True)
            if got != want:
                problems.append("%s %s: the library splits %d ways, the restated 32-wide geometry %d" % (fam, name, got, want))
            changed += want != E.wgrad_x3_ksplit(B, H, W, C0 + C1, Co)
    if not changed:
        problems.append("no case changes its split count under the switch")
    for name, (shape, expect, tiles16, _) in E.WGX3_TW32_CASES.items():
        B, C0, C1, Co, H, W = shape
        g = E.wgrad_x3_geometry(B, H, W, C0 + C1, Co, tw32=True)
        problems += ["%s: %s is %r, listed as %r" % (name, k, g[k], v) for k, v in expect.items() if g[k] != v]
    return {"cases_with_another_split_count": changed}, problems


def prove_tail0(L):
    """A host query cannot see WTPSE_TAIL_MAX_WGS: the proof is each call's own — poisoned tickets that come back untouched
    (test_conv_x3_gpu.tail_forward / tail_backward)."""
    ok = os.environ.get("WTPSE_TAIL_MAX_WGS") == "0"
    return {"by": "poisoned tickets, per call"}, ([] if ok else ["WTPSE_TAIL_MAX_WGS is not 0 in this process"])


def prove(L, job):
    name, value, _ = S.JOBS[job]
    if os.environ.get(name) != value:
        return {}, ["%s=%s is not set in this process" % (name, value)]
    if job == "tw32":
        return prove_tw32(L)
    if job == "tail0":
        return prove_tail0(L)
    return prove_x3(L, job)


# =============================================================================================== the GPU side
def run_tw32():
    import test_exact_conv_gpu as G
    failures, calls = [], 0
    for fam in ("x3", "x3tw32"):
        for name in E.wgrad_cases(fam):
            failures += G.wgrad_failures(fam, name, G.all_modes)
            calls += 1
            G._DEV.clear()
            E.clear_caches()
    return failures, calls


def run_x3(job):
    import test_exact_conv_gpu as G
    failures, calls = [], 0
    for table, idx in x3_job_cases(job):
        for cls in (("I",) if job == "mt1" else E.CONV_CLASSES):
            failures += G.x3_failures(table, idx, cls, X3R_SETTINGS[table])
            calls += 1
        G._DEV.clear()
        E.clear_caches()
    return failures, calls


# layout, (B, C0, C1, Cout, H, W, k): the small shapes of test_conv_fwd_bnf / test_dgrad_bnb, one input
TAIL0_FORWARD = [(1, (2, 16, 0, 32, 16, 16, 3)), (1, (3, 64, 0, 96, 8, 16, 1)), (1, (3, 16, 0, 32, 10, 32, 3)), (0, (3, 3, 0, 16, 24, 40, 3)),
                 (0, (4, 8, 0, 40, 16, 32, 1)), (2, (3, 16, 0, 16, 24, 40, 3))]
TAIL0_BACKWARD = [(0, (3, 16, 0, 16, 24, 40, 3)), (0, (2, 32, 0, 32, 16, 32, 3)), (0, (2, 16, 0, 16, 20, 20, 1)), (1, (2, 32, 0, 32, 16, 32, 3)),
                  (1, (4, 64, 0, 64, 16, 16, 3)), (1, (2, 64, 0, 128, 8, 8, 1))]


def bnb_tail_failures(idx, frozen):
    """One case of the bnb table in class I through wtpse_dgrad_bnb_coef[_frozen] in every layout it runs in, behind poisoned tickets:
    masked gradient, other half and partials against the fp64 reference (bits), coefficients and gradients against the stand-alone
    fold of the call's own partials (bits)."""
    import torch
    import test_conv_x3_gpu as TX
    import test_exact_conv_gpu as G
    from test_kernels_gpu import ops, pack, DEV
    o = ops()
    L, ptr, st = o.lib(), o.ptr, o.stream_ptr()
    case = E.TABLES["bnb"][idx]
    B, Cl, Co, bn_second, Cn, H, W, k, relu, _ = case
    Ct = Cl + Co
    p = E.bnb_problem(idx, "I")
    failures = []
    gamma = (torch.arange(Cl, dtype=torch.float32) * 0.37 + 0.5).to(DEV)
    invstd = (torch.arange(Cl, dtype=torch.float32) * 0.11 + 0.7).to(DEV)
    for layout in E.bnb_layouts(case):
        w = p["w"].float()
        packed, _, off = pack(w) if layout == 0 else (TX.pack_x3(w) if layout == 1 else TX.pack_x16(w))
        wptr = packed.data_ptr() + (4 if layout == 0 else 2) * off
        du, y, ss, mean = G.dev(p["du"]), G.dev(p["y"]), G.dev(p["ss"]), G.dev(p["mean"])
        if p["split"] is None:
            out0, out1, csplit = G.sentinel(B, Ct, H, W), None, Ct
        else:
            csplit = p["split"]
            out0, out1 = G.sentinel(B, csplit, H, W), G.sentinel(B, Ct - csplit, H, W)
        nblk = o._stats_blocks(layout, B, H, W, Ct, k)
        stats = G.sentinel(nblk, Cl, 2)
        tickets, partial2 = TX._tail_buffers(nblk, Ct)
        coef, dg, dbt, dbias = G.sentinel(Cl, 3), G.sentinel(Cl), G.sentinel(Cl), G.sentinel(Cl)
        args = [ptr(du), Cn, wptr, layout, ptr(out0), ptr(out1), csplit, ptr(y), ptr(ss), ptr(mean), int(relu), p["c0"], p["c1"], ptr(stats),
                ptr(gamma), ptr(invstd), ptr(coef), ptr(dg), ptr(dbt)] + ([ptr(dbias)] if frozen else [])
        L.call("wtpse_dgrad_bnb_coef_frozen" if frozen else "wtpse_dgrad_bnb_coef", *args, 0, ptr(partial2), ptr(tickets), B, H, W, Ct, k, 0, st)
        torch.cuda.synchronize()
        what = "dgrad_bnb_coef%s %s layout %d class I" % ("_frozen" if frozen else "", case, layout)
        if not bool((tickets == TX.POISON).all()):
            failures.append(what + ": the tickets were touched — the launch folded in place, WTPSE_TAIL_MAX_WGS=0 is not in force")
        for f in (G.differs(out1 if (Co and bn_second) else out0, p["g"], what + ": masked gradient (image, channel, row, column)"),
                  G.differs(out0 if bn_second else out1, p["other"], what + ": other half") if Co else None,
                  G.differs(stats, p["stats"], what + ": partials (channel, [sum g, sum g (y - mean)])", rows=True)):
            if f:
                failures.append(f)
        coef2, dg2, dbt2, dbias2 = G.sentinel(Cl, 3), G.sentinel(Cl), G.sentinel(Cl), G.sentinel(Cl)
        if frozen:
            L.call("wtpse_bn_bwd_finalize_coef_frozen", ptr(stats), nblk, Cl, ptr(gamma), ptr(invstd), ptr(coef2), ptr(dg2), ptr(dbt2), ptr(dbias2), 0, st)
        else:
            L.call("wtpse_bn_bwd_finalize_coef", ptr(stats), nblk, Cl, B * H * W, ptr(gamma), ptr(mean), ptr(invstd), ptr(coef2), ptr(dg2),
                   ptr(dbt2), 0, st)
        torch.cuda.synchronize()
        for name, a_, b_ in (("coef", coef, coef2), ("dgamma", dg, dg2), ("dbeta", dbt, dbt2)) + ((("dbias", dbias, dbias2),) if frozen else ()):
            if not bool(torch.isfinite(b_).all()):
                failures.append(what + ": " + name + " of the stand-alone fold is not finite")
            TX._same(what + ": " + name, a_, b_, failures)
    G._DEV.clear()
    E.clear_caches()
    return failures


def run_tail0():
    import test_conv_x3_gpu as TX
    import test_dispatch_paths_gpu as DP
    failures, calls = [], 0
    for layout, case in TAIL0_FORWARD:
        failures += TX.tail_forward(layout, case, after=True)
        calls += 1
    for layout, case in TAIL0_BACKWARD:
        for frozen in (False, True):
            failures += TX.tail_backward(layout, case, frozen)
            calls += 1
    for idx in range(len(E.TABLES["bnb"])):
        for frozen in (False, True):
            failures += bnb_tail_failures(idx, frozen)
            calls += 1
    for form in ("tail", "tail_frozen"):           # against bn_finish_ref within its derived bounds (asserts)
        try:
            DP.test_batchnorm_backward_finishers_on_exact_sums(form)
        except AssertionError as e:
            failures.append("BN_EXACT_FORMS %s: %s" % (form, e))
        calls += 1
    return failures, calls


def main(argv):
    job, out_path = argv[1], argv[2]
    host = "--host" in argv[3:]
    t0 = time.time()
    L = lib()
    proof, problems = prove(L, job)
    res = {"job": job, "proof": proof, "failures": ["switch not proved in force: " + p for p in problems], "calls": 0}
    if not problems and not host:
        import torch
        assert torch.cuda.is_available(), "the job needs the GPU"
        failures, calls = run_tw32() if job == "tw32" else run_tail0() if job == "tail0" else run_x3(job)
        torch.cuda.synchronize()
        res.update(failures=failures, calls=calls)
    res["seconds"] = round(time.time() - t0, 2)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("switch_worker %s: %d failure(s), %d case runs, %.1f s" % (job, len(res["failures"]), res["calls"], res["seconds"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
