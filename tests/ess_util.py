"""What tests/test_ess.py (host-emulation build) and tests/test_ess_gpu.py (-m gpu, the product libraries) share: the plain-Python
restatements of include/gphocs_hip.h's effective-sample-size definitions -- gph_ess_add, gph_ess_read, gph_ess, and the M series
k_ess keeps per locus, rebuilt from the same chain's gene-tree records -- and the check_* functions both files call.

Nothing here has a tolerance except the one sanity bound on tau the definitions come with: every comparison is float.hex
against float.hex, and counts, focal sets and selections are compared exactly."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import compare_records
from sampler_util import load_pack

J = 16                  # GPH_ESS_LEVELS
WORDS = 2 + 2 * J
FULL, EARG, ESTATE = -5, -1, -4
CLS = 21                # timing class of k_ess
GT_O_DATALNL = 3        # gph_engine_gene_trees_shape: the offset of dataLnL in a record; FS_MUTRATE lies 4 doubles behind it
CHECKPOINTS = (1, 2, 37, 64)      # S = 1, S = 2, incomplete tails at every level, every run[j] = 0


# ---------------------------------------------------------------- the definitions restated
def ess_add(a, t, x):
    if t == 0:
        for i in range(WORDS):
            a[i] = 0.0
        a[0] = x
    d = 0.0 if t == 0 else x - a[0]
    a[1] = a[1] + d
    a[2 + J] = a[2 + J] + d * d
    carry = d
    for j in range(1, J):
        a[2 + j] = a[2 + j] + carry
        if (t + 1) % (1 << j) != 0:
            break
        carry = a[2 + j]
        a[2 + J + j] = a[2 + J + j] + carry * carry
        a[2 + j] = 0.0


def level_for(S):
    j = 0
    while j + 1 < J and 4 ** (j + 1) <= S:
        j += 1
    return j


def ess_read(a, S, level=-1):
    """(mean, sd, tau, ess, level)"""
    j = level_for(S) if level < 0 else level
    if S < 1:
        return 0.0, 0.0, 0.0, 0.0, j
    s1, n = a[1], float(S)
    mean = a[0] + s1 / n
    if S < 2:
        return mean, 0.0, 0.0, 0.0, j
    vx = (a[2 + J] - s1 * s1 / n) / float(S - 1)
    sd = float(np.sqrt(vx)) if vx > 0.0 else 0.0
    if not vx > 0.0:
        return mean, sd, 0.0, 0.0, j
    b = 1 << j
    nb = S // b
    tau = 0.0
    if nb >= 2:
        tail = 0.0
        for i in range(1, j + 1):
            tail = tail + a[2 + i]
        T = s1 if j == 0 else s1 - tail
        vb = (a[2 + J + j] - T * T / float(nb)) / float(nb - 1)
        tau = vb / (float(b) * vx)
    ess = n
    if tau > 0.0:
        ess = n / tau
        if ess > n:
            ess = n
    return mean, sd, tau, ess, j


def _ordered_sum(p):
    """p[0] + p[1] + ... in index order from 0.0 (np.add.accumulate forms every prefix, so it cannot reorder)"""
    return float(np.add.accumulate(p)[-1]) if len(p) else 0.0


def ess_series(x, max_lag=0):
    """gph_ess restated: the dict gphocs_amd.ess returns"""
    x = [float(v) for v in x]
    S = len(x)
    a = [0.0] * WORDS
    for t, v in enumerate(x):
        ess_add(a, t, v)
    mean, sd, tau_b, ess_b, level = ess_read(a, S)
    n = float(S)
    m = a[1] / n
    e = np.array([(0.0 if t == 0 else x[t] - x[0]) - m for t in range(S)], dtype=np.float64)

    def cov(k):
        return _ordered_sum(e[k:] * e[:S - k]) / n
    kmax = min(S - 2, 2000 if max_lag <= 0 else max_lag)
    c0 = cov(0)
    total, truncated, i = c0 + cov(1), 0, 1
    while True:
        if 2 * i + 1 > kmax:
            truncated = 1
            break
        g = cov(2 * i) + cov(2 * i + 1)
        if not g > 0.0:
            break
        total = total + g
        i += 1
    tau, ess = 0.0, 0.0
    if c0 != 0.0:
        tau = 2.0 * total / c0 - 1.0
        ess = n
        if tau > 0.0:
            ess = n / tau
            if ess > n:
                ess = n
    return dict(mean=mean, sd=sd, tauBatch=tau_b, essBatch=ess_b, tauAcf=tau, essAcf=ess, level=level, truncated=truncated)


def ar1(S, phi, seed):
    """x_t = phi x_t-1 + u_t with u_t from a fixed integer generator (a 64-bit LCG's top 53 bits, twelve of them summed:
    variance 1): the same doubles on every platform"""
    state = seed & ((1 << 64) - 1)
    out, x = [], 0.0
    for _ in range(S):
        u = -6.0
        for _ in range(12):
            state = (state * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
            u = u + (state >> 11) / 9007199254740992.0
        x = phi * x + u
        out.append(x)
    return out


def same_bits(got, want, what):
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, float):
            assert float(g).hex() == float(w).hex(), f"{what}: {k}: {g!r} != {w!r}"
        else:
            assert g == w, f"{what}: {k}: {g!r} != {w!r}"


# ---------------------------------------------------------------- the model of k_ess: plain Python over decoded gene-tree records
def clade_masks(father, n):
    N = 2 * n - 1
    mask = [0] * N
    for i in range(n):
        v = i
        for _ in range(N):
            f = father[v]
            if not n <= f < N:
                break
            mask[f] |= 1 << i
            v = f
    return mask[n:]


def model_loci(t, n, M, rates, S):
    """per selected locus over the first S samples of the gene-tree records t: dict(acc [M][WORDS], focal [n - 1] keys,
    changes)"""
    Q = t["father"].shape[1]
    out = []
    for q in range(Q):
        acc = [[0.0] * WORDS for _ in range(M)]
        focal, fset, prev, changes = None, None, None, 0
        for s in range(S):
            keys = clade_masks(t["father"][s, q].tolist(), n)
            if s == 0:
                focal, fset = keys, set(keys)
            else:
                changes += set(keys) != prev          # clade SETS compared, no hash
            prev = set(keys)
            x = [float(t["dataLnL"][s, q]), float(t["genLnL"][s, q]), float(t["age"][s, q, int(t["root"][s, q])]), float(int(t["num_migs"][s, q])),
                 float(sum(k in fset for k in keys))]
            if M > 5:
                x.append(float(rates[s, q]))
            for m in range(M):
                ess_add(acc[m], s, x[m])
        out.append(dict(acc=acc, focal=focal, changes=changes))
    return out


def run_chain(lib, name, iters, loci=None, checkpoints=(), sample=True, trees=True, record=None, final=None, pack=None):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees and of k_ess after
    every iteration; Sampler.ess() is fetched (no reset) after each of `checkpoints` samples and at the end"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.ess_enable(loci)
        s.initialize()
        hs0 = s.host_stats()
        at = {}
        for it in range(iters):
            s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                s.ess_sample()
                if it + 1 in checkpoints:
                    at[it + 1] = s.ess()
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        if sample:
            at[iters] = s.ess()
        t = rates = None
        if sample and trees:
            off = s._gene_trees_shape()[3][GT_O_DATALNL]
            t = s.gene_trees(raw=True)
            rec = t["records"]
            rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[:, :, 0] if rec.size else np.zeros(rec.shape[:2])
        if final:
            s.dump_state(final, True)
        return dict(ess=at, trees=t, rates=rates, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob())
    finally:
        s.close()


def check_against_model(e, t, rates, n, S, what, rows=None):
    """item 1: what Sampler.ess() fetched after S samples against the model over the first S records (rows: the records' loci
    that the fetched selection holds, None: the same selection); item 3: the table against ess_read over the fetched words"""
    Q, M = len(e["loci"]), len(e["series"])
    assert e["samples"] == S and e["levels"] == J and e["words"] == (n + 63) // 64
    assert e["acc"].shape == (Q, M, WORDS) and e["focal"].shape == (Q, n - 1, e["words"]) and e["changes"].shape == (Q,)
    rows = list(range(Q)) if rows is None else rows
    model = model_loci(t, n, M, rates, S)
    for q, r in enumerate(rows):
        m, g = model[r], int(e["loci"][q])
        for k in range(M):
            got, want = [float(v).hex() for v in e["acc"][q, k]], [float(v).hex() for v in m["acc"][k]]
            assert got == want, f"{what} S {S}: locus {g} series {e['series'][k]}: words {[i for i in range(WORDS) if got[i] != want[i]]} differ"
        focal = [sum(int(e["focal"][q, k, w]) << (64 * w) for w in range(e["words"])) for k in range(n - 1)]
        assert focal == m["focal"], f"{what} S {S}: locus {g}: the focal set"
        assert int(e["changes"][q]) == m["changes"], f"{what} S {S}: locus {g}: topoChanges {int(e['changes'][q])} != {m['changes']}"
    check_table(e, what)
    return model


def check_table(e, what, level=-1):
    Q, M, S = len(e["loci"]), len(e["series"]), e["samples"]
    assert e["level"] == (level_for(S) if level < 0 else level)
    for q in range(Q):
        ess_moved = []
        for k in range(M):
            mean, sd, tau, ess, _ = ess_read([float(v) for v in e["acc"][q, k]], S, level)
            got = dict(mean=float(e["mean"][q, k]), sd=float(e["sd"][q, k]), tau=float(e["tau"][q, k]), ess=float(e["ess"][q, k]))
            same_bits(got, dict(mean=mean, sd=sd, tau=tau, ess=ess), f"{what}: locus {int(e['loci'][q])} series {e['series'][k]}")
            if sd > 0.0:
                ess_moved.append(ess)
        assert float(e["min_ess"][q]) == (min(ess_moved) if ess_moved else 0.0)


def check_case(lib, name, iters=64, checkpoints=CHECKPOINTS, key="cpu"):
    """item 1 for one case: every fetch at the checkpoints against the model over the chain's own records"""
    cps = [c for c in checkpoints if c <= iters]
    r = run_chain(lib, name, iters, checkpoints=cps)
    n, t = r["pack"].n, r["trees"]
    assert r["launches"] == iters and r["oob"][0] == 0
    assert sorted(r["ess"]) == sorted(set(cps + [iters]))
    for S, e in sorted(r["ess"].items()):
        assert e["loci"].tolist() == list(range(r["pack"].L)) == t["loci"].tolist()
        model = check_against_model(e, t, r["rates"], n, S, name)
    moved = sum(m["changes"] > 0 for m in model)
    print(f"{name} [{key}] n {n} loci {len(model)} series {len(e['series'])} samples {iters}: loci whose topology changed {moved}, "
          f"topoChanges {sorted(m['changes'] for m in model)[::max(1, len(model) // 8)]}")
    return r, model


def check_selections(lib, name="x8", iters=9):
    """item 1, selections: all loci; one locus; a stride off the group size; the last locus alone -- each row equals the same
    locus's row of the all-loci model.  The usage errors of the selection, and a rank without a selected locus"""
    import gphocs_amd as G
    everything = run_chain(lib, name, iters)
    pk, t = everything["pack"], everything["trees"]
    n, L = pk.n, pk.L
    per_group = max(1, 256 // n)
    assert 2 <= per_group < L, "the case has too few loci for a group and one more"
    check_against_model(everything["ess"][iters], t, everything["rates"], n, iters, f"{name} all")
    for sel in ([3], list(range(0, L, 3)), [L - 1], list(range(per_group + 1))):
        assert per_group % 3 != 0
        r = run_chain(lib, name, iters, loci=sel, trees=False)
        e = r["ess"][iters]
        assert e["loci"].tolist() == sel and r["launches"] == iters
        check_against_model(e, t, everything["rates"], n, iters, f"{name} selection {sel}", rows=sel)
    s = G.Sampler(pk, lib=lib)
    try:
        for bad in ([3, 2], [2, 2], [-1], [0, -1]):
            with pytest.raises(ValueError):
                s.ess_enable(bad)
            assert s.lib.gph_engine_ess_enable(s.engine, (ctypes.c_int64 * len(bad))(*bad), len(bad), 0) == EARG
        s.ess_enable([L + 5])          # beyond the rank's block: ignored -- the rank counts its samples and launches nothing
        s.initialize()
        n0 = s.host_stats()["launches"]
        s.ess_sample()
        s.ess_sample()
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == 0
        e = s.ess()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["acc"].shape == (0, 5, WORDS)
    finally:
        s.close()


def check_levels(lib, name="m3", counts=(3, 4, 15, 16, 17)):
    """item 3: the level rule where it steps (4^1 = 4, 4^2 = 16), and every explicit level, on one chain"""
    import gphocs_amd as G
    s = G.Sampler(load_pack(name), lib=lib)
    try:
        s.ess_enable()
        s.initialize()
        for it in range(max(counts)):
            s.iteration(it)
            s.ess_sample()
            if it + 1 in counts:
                e = s.ess()
                assert e["level"] == {3: 0, 4: 1, 15: 1, 16: 2, 17: 2}[it + 1]
                check_table(e, f"{name} S {it + 1}")
        for level in range(J):
            check_table(s.ess(level=level), f"{name} level {level}", level)
        with pytest.raises(ValueError):
            s.ess(level=J)
        before = s.ess()                           # the same state sampled again: no topology change is counted
        s.ess_sample()
        after = s.ess()
        assert after["samples"] == before["samples"] + 1 and after["changes"].tolist() == before["changes"].tolist()
        assert before["changes"].any() and after["focal"].tobytes() == before["focal"].tobytes()
    finally:
        s.close()


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12):
    """item 4: records and final state dump with sampling on identical to a run with sampling off, and still the reference's
    records; launches of class 21 = the samples.  Returns the two runs"""
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        r = run_chain(lib, name, full, sample=on, trees=False, record=rec, final=final, pack=__import__("gphocs_amd").Pack.load(os.path.join(GOLDEN, name + ".gpk")))
        out.append(dict(rec=rec, final=final, stats=r["stats"], launches=r["launches"], samples=r["ess"][full]["samples"] if on else 0))
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    return on, off


def check_lifecycle(lib, G, name="m3", iters=5):
    """item 6: reset, re-enable, GPH_EFULL with nothing allocated, GPH_ESTATE"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    n, L = pk.n, pk.L
    need = L * (5 * WORDS * 8 + (n - 1) * 8 + 8 + 4)
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.ess()                                    # not enabled
        assert s.lib.gph_engine_ess_fetch(s.engine, None, None, None, 0) == ESTATE
        assert s.lib.gph_engine_ess_sample(s.engine) == ESTATE
        assert s._ess_shape() == (0, 0, 0, 0, 0)
        s.ess_enable()
        assert s._ess_shape() == (L, 5, J, 1, 0)
        assert s.lib.gph_engine_ess_sample(s.engine) == ESTATE          # before initialize
        assert s.lib.gph_engine_ess_enable(s.engine, None, 0, need - 1) == FULL
        assert s._ess_shape() == (0, 0, 0, 0, 0)       # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.ess_enable(max_bytes=need - 1)
        s.initialize()                                 # the engine is still usable
        with pytest.raises(RuntimeError):
            s.ess_sample()
        s.ess_enable([1, 2])                           # re-enable: another selection, then the real one
        assert s._ess_shape() == (2, 5, J, 1, 0)
        s.ess_enable(max_bytes=need)
        for it in range(iters):
            s.iteration(it)
            s.ess_sample()
        first = s.ess(reset=True)
        assert first["samples"] == iters and n <= 64
        assert all((1 << n) - 1 in first["focal"][q, :, 0].tolist() for q in range(L))       # the root's clade is in every focal set
        zero = s.ess()
        assert zero["samples"] == 0 and not zero["acc"].view(np.uint64).any() and not zero["focal"].any() and not zero["changes"].any()
        assert not zero["ess"].any() and not zero["min_ess"].any()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.ess_sample()
        second = s.ess()
        s2 = G.Sampler(pk, lib=lib)                    # the same chain, sampled over the second half only
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.ess_enable()
                s2.iteration(it)
                if it >= iters:
                    s2.ess_sample()
            fresh = s2.ess()
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert second["acc"].tobytes() == fresh["acc"].tobytes() != first["acc"].tobytes()
        assert second["focal"].tobytes() == fresh["focal"].tobytes() and second["changes"].tolist() == fresh["changes"].tolist()
        s.initialize()                                 # a new chain starts from zeroed accumulators
        again = s.ess()
        assert again["samples"] == 0 and not again["acc"].view(np.uint64).any() and not again["changes"].any()
    finally:
        s.close()


# ---------------------------------------------------------------- the program and the launcher (item 5)
def _g(x):
    return "%.10g" % x


def expected_files(ctl_dir, ctl, header, spec_loci, lib=None, sampler_lib=None):
    """the text of PREFIX.ess.tsv and PREFIX.locus-ess.tsv the program must write: an equivalent Sampler run (burn-in first, a
    sample wherever a trace line is written), the trace columns through ess_series, the fetched accumulators through ess_read"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    npar = p.numParameters
    pf = np.asarray(p.printFactors, dtype=np.float64)
    x = []
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.ess_enable(spec_loci)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it >= 0 and it % (p.sampleSkip + 1) == 0:
                s.ess_sample()
                v = np.zeros(npar + 4)
                assert s.lib.gph_mcmc_param_vals(s.mcmc, v.ctypes.data, npar) == 0
                st = s.state()
                x.append([float(v[i] * pf[i]) for i in range(npar)] + [st["logLikelihood"], st["dataLogLikelihood"]])
        e = s.ess()
    finally:
        s.close()
    S = len(x)
    assert len(header) == npar + 2 and e["samples"] == S
    level = level_for(S)
    rows, worst = ["\t".join(["param", "samples", "mean", "sd", "essBatch", "essAcf", "tauAcf", "truncated"])], None
    for i, name in enumerate(header):
        r = ess_series([x[t][i] for t in range(S)])
        rows.append("\t".join([name, str(S), _g(r["mean"]), _g(r["sd"]), _g(r["essBatch"]), _g(r["essAcf"]), _g(r["tauAcf"]), str(r["truncated"])]))
        if r["sd"] > 0.0 and (worst is None or r["essAcf"] < worst[0]):
            worst = (r["essAcf"], name)
    params = "samples %d level %d batch %d minEssAcf %s (%s)" % (S, level, 1 << level, _g(worst[0] if worst else 0.0), worst[1] if worst else "-")
    rows.append("# " + params)
    M = len(e["series"])
    loci = ["\t".join(["locus", "name", "samples"] + ["ess" + nm[0].upper() + nm[1:] for nm in e["series"]] + ["topoChanges", "minEss"])]
    least = []
    for q, g in enumerate(e["loci"].tolist()):
        r = [ess_read([float(v) for v in e["acc"][q, m]], S) for m in range(M)]
        moved = [t[3] for t in r if t[1] > 0.0]
        least.append((min(moved) if moved else 0.0, g))
        loci.append("\t".join([str(g), p.locusNames[g], str(S)] + [_g(t[3]) for t in r] + [str(int(e["changes"][q])), _g(least[-1][0])]))
    v = sorted(t[0] for t in least)
    Q = len(v)
    median = 0.0 if Q == 0 else v[Q // 2] if Q % 2 else (v[Q // 2 - 1] + v[Q // 2]) / 2.0
    lo = min(least, key=lambda t: t[0]) if least else (0.0, -1)        # (the first of equal ones, as the program takes it)
    tail = "loci %d level %d batch %d medianMinEss %s minMinEss %s (locus %d)" % (Q, level, 1 << level, _g(median), _g(lo[0]), lo[1])
    loci.append("# " + tail)
    return "\n".join(rows) + "\n", "\n".join(loci) + "\n", f"ESS: {params}; {tail}"


def check_program(lib_path, lib, tmp_path):
    """both files are the restatement over an equivalent Sampler run, character for character, and the log repeats their summary
    lines; the other options' files do not move; with --mc3 (no swaps) and --replicates the files are chain 0's = the plain
    run's; readTrace --ess; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import PROGRAM_CASE, PROGRAM_LOCI, PROGRAM_SPEC, program_ctl
    name = PROGRAM_CASE
    ctl = name + ".ctl"
    a, b, d, e, m, r = (tmp_path / x for x in ("with", "without", "all", "rest", "mc3", "rep"))
    for x in (a, b, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    run = _run(lib_path, a, ["--ess", "out", "--ess-loci", PROGRAM_SPEC, ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["ess.tsv", "locus-ess.tsv"]                   # no part left behind
    header = open(trace).readline().rstrip("\n").split("\t")[1:]
    want_params, want_loci, want_log = expected_files(str(a), ctl, header, PROGRAM_LOCI, lib, lib)
    assert got["ess.tsv"] == want_params
    assert got["locus-ess.tsv"] == want_loci
    assert want_log in run.stdout.splitlines()
    assert [int(ln.split("\t")[0]) for ln in got["locus-ess.tsv"].splitlines()[1:-1]] == PROGRAM_LOCI
    # the other outputs do not move
    rest = ["-l", "sum.tsv", "--clades", "cl", "--clades-loci", "1-5", "--gene-trees", "gt", "--gene-trees-loci", "1-5"]
    _run(lib_path, d, ["--ess", "out", "--ess-loci", PROGRAM_SPEC] + rest + [ctl])
    _run(lib_path, e, rest + [ctl])
    assert read_outputs(d, "out") == got
    assert open(d / "sum.tsv").read() == open(e / "sum.tsv").read()
    for prefix, count in (("cl", 2), ("gt", 1)):
        other = read_outputs(e, prefix)
        assert len(other) == count and read_outputs(d, prefix) == other
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # chain 0 of a group of chains is the plain run's chain
    _run(lib_path, m, ["--mc3", "2", "--mc3-swap-every", "-1", "--ess", "out", "--ess-loci", PROGRAM_SPEC, ctl])
    assert read_outputs(m, "out") == got
    _run(lib_path, r, ["--replicates", "2", "--replicates-out", "rep", "--ess", "out", "--ess-loci", PROGRAM_SPEC, ctl])
    assert read_outputs(r, "out") == got
    # readTrace --ess: gph_ess over the parsed file (what %f printing of the trace keeps), and next to the run's own table
    tool = os.path.join(os.path.dirname(EXE), "readTrace")
    out = subprocess.run([tool, str(trace), "--ess"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    cols = np.array([[float(v) for v in ln.split()[1:]] for ln in open(trace).read().splitlines()[1:]], dtype=np.float64)
    S = cols.shape[0]
    lines = out.stdout.splitlines()
    assert lines[0] == got["ess.tsv"].splitlines()[0] and len(lines) == len(header) + 2
    worst = None
    for i, nm in enumerate(header):
        w = G.ess(cols[:, i], lib=lib or G.load_library())
        assert lines[1 + i] == "\t".join([nm, str(S), _g(w["mean"]), _g(w["sd"]), _g(w["essBatch"]), _g(w["essAcf"]), _g(w["tauAcf"]), str(w["truncated"])])
        if w["sd"] > 0.0 and (worst is None or w["essAcf"] < worst[0]):
            worst = (w["essAcf"], nm)
        mine = got["ess.tsv"].splitlines()[1 + i].split("\t")
        assert mine[:2] == [nm, str(S)] and abs(float(mine[2]) - w["mean"]) <= 1e-5 * max(1.0, abs(w["mean"]))      # (%8.5f / %.6f printing)
    assert lines[-1] == "# samples %d level %d batch %d minEssAcf %s (%s)" % (S, level_for(S), 1 << level_for(S), _g(worst[0]), worst[1])
    skipped = subprocess.run([tool, str(trace), "--ess", "-d", "4"], capture_output=True, text=True, timeout=600)
    assert skipped.returncode == 0 and skipped.stdout.splitlines()[1].split("\t")[1] == str(S - 4)
    plain = subprocess.run([tool, str(trace)], capture_output=True, text=True, timeout=600)
    size, err = ctypes.c_size_t(), ctypes.create_string_buffer(512)
    anylib = lib or G.load_library()
    anylib.gph_read_trace(str(trace).encode(), -1, 0, None, 0, ctypes.byref(size), err, 512)
    buf = ctypes.create_string_buffer(size.value + 1)
    assert anylib.gph_read_trace(str(trace).encode(), -1, 0, buf, size.value + 1, ctypes.byref(size), err, 512) == 0
    assert plain.returncode == 0 and plain.stdout == buf.value.decode() and "essAcf" not in plain.stdout
    # usage errors: they name the option, before anything is read, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    L = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).L
    on = ["--ess", "out"]
    for args, word in ((["--ess-loci", "0-3"], "--ess"), (on + ["--ess-loci", "0-4,3"], "locus 3 "), (on + ["--ess-loci", "5,5"], "locus 5 "),
                       (on + ["--ess-loci", f"3,{L}"], f"locus {L} "), (on + ["--ess-loci", "2-x"], "2-x")):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and word in res.stderr and "--ess-loci" in res.stderr, (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        assert G.run_control_file(lib or G.load_library(dims=(p.n, p.K, p.B)), ctl, ess_loci="0-3") == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, concatenated by gph_ess_write, are the one-rank files -- for all loci, and for a selection
    that lies wholly in rank 1's block; the launcher does the same; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, ess="out", ess_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["ess.tsv", "locus-ess.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["locus-ess.tsv"].splitlines()[1:-1]] == loci
        run_ranks(lib_path, name, 2, two, ess="out", ess_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.ess.part0", "out.ess.part1"]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.ess.part{r}", cut)
            text = open(cut / "out.ess.part1").read().splitlines(True)
            open(cut / "out.ess.part1", "w").write("".join(text[:-1]))
            assert lib.gph_ess_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_ess_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                          # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--ess", "out", "--ess-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.locus-ess.tsv must be written:
    status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.locus-ess.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--ess", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.locus-ess.tsv"] and not os.listdir(d / "out.locus-ess.tsv")
