"""What tests/test_simulate.py (host-emulation build) and tests/test_simulate_gpu.py (-m gpu, the product libraries) share: a
plain-Python restatement of include/gphocs_hip.h's definition of the replicate genealogies -- the generator, the event loop,
the record, the statistics, the accumulators -- and the check_* functions both files call.  The restatement computes with
Python floats (IEEE doubles, one rounding an operation) and math.log (glibc's); nothing here calls the library to compute what it
checks, and nothing has a tolerance: ages are compared as bit patterns, accumulator words as float.hex, rows as integers."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import compare_records
from predictive_util import EARG, ESTATE, FULL, M64, columns, leaf_pops, mix_int, observed, replicate, stat_names, statistics
from sampler_util import load_pack

CLS = 25                # timing class of k_simulate (and the site loop behind it)
CHECKPOINTS = (1, 2, 9)
DOMAIN, ATTEMPT, SITES, GOLD = 0x53494D554C415445, 0xD1B54A32D192ED03, 0x5349544553, 0x9E3779B97F4A7C15
ATTEMPTS, MAX_MIGS = 16, 10
INF = float("inf")


# ---------------------------------------------------------------- the definitions restated
def locus_key(seed, g):
    return mix_int((seed ^ DOMAIN) ^ mix_int(g + GOLD))


def attempt_key(seed, g, t, a):
    return mix_int(mix_int(locus_key(seed, g) + t) + (a + 1) * ATTEMPT)


def site_key(seed, g, t):
    return mix_int(locus_key(seed ^ SITES, g) + t)


class Draws:
    def __init__(self, ka):
        self.ka, self.d = ka, 0

    def __call__(self):
        h = mix_int(self.ka ^ self.d)
        self.d += 1
        return (float(h >> 12) + 0.5) * 2.0 ** -52


def make_model(n, Kc, popFather, leafpop, theta, popAge, sampleAge, bandSrc=(), bandTgt=(), migRate=(), bandStart=(), bandEnd=()):
    K, B = len(popFather), len(bandSrc)
    assert len(theta) == len(popAge) == len(sampleAge) == K and len(leafpop) == n
    assert len(bandTgt) == len(migRate) == len(bandStart) == len(bandEnd) == B
    return dict(n=n, N=2 * n - 1, K=K, Kc=Kc, B=B, popFather=[int(x) for x in popFather], leafpop=[int(x) for x in leafpop],
                theta=[float(x) for x in theta], popAge=[float(x) for x in popAge], sampleAge=[float(x) for x in sampleAge],
                bandSrc=[int(x) for x in bandSrc], bandTgt=[int(x) for x in bandTgt], migRate=[float(x) for x in migRate],
                bandStart=[float(x) for x in bandStart], bandEnd=[float(x) for x in bandEnd])


def attempt(m, ka):
    """one attempt: (0, replicate) | (1, None) abandoned at the migration cap | (2, None) no way on"""
    n, N, K, Kc, B = m["n"], m["N"], m["K"], m["Kc"], m["B"]
    draw = Draws(ka)
    age, father, left, right, npop = [0.0] * N, [0] * N, [0] * N, [0] * N, [0] * N
    lin = []                                    # [node, population]
    entered = [False] * Kc
    ncoal, nmig, coalst, migst, migs = [0] * K, [0] * B, [0.0] * K, [0.0] * B, []

    def enter(t):
        for p in range(Kc):
            if entered[p] or not m["sampleAge"][p] <= t:
                continue
            entered[p] = True
            for i in range(n):
                if m["leafpop"][i] == p:
                    lin.append([i, p])
                    age[i], father[i], left[i], right[i], npop[i] = m["sampleAge"][p], -1, -1, -1, p
        for ln in lin:
            for _ in range(K):
                F = m["popFather"][ln[1]]
                if not 0 <= F < K or not m["popAge"][F] <= t:
                    break
                ln[1] = F

    def rates(t):
        """(index, rate, count) of the non-zero rates in walk order"""
        out = []
        for p in range(K):
            c = sum(1 for ln in lin if ln[1] == p)
            if c >= 2:
                r = float(c * (c - 1)) / m["theta"][p]
                if r != 0.0:
                    out.append((p, r, c))
        for b in range(B):
            if m["bandStart"][b] <= t < m["bandEnd"][b]:
                c = sum(1 for ln in lin if ln[1] == m["bandTgt"][b])
                if c >= 1:
                    r = float(c) * m["migRate"][b]
                    if r != 0.0:
                        out.append((K + b, r, c))
        return out

    t, nco = 0.0, 0
    enter(t)
    for _ in range(n + MAX_MIGS + K + Kc + 2 * B + 8):
        if len(lin) == 1 and all(entered):
            return 0, dict(age=age, father=father, left=left, right=right, npop=npop, migs=migs, ncoal=ncoal, nmig=nmig, coalst=coalst, migst=migst,
                           draws=draw.d)
        rs = rates(t)
        R = 0.0
        for _, r, _ in rs:
            R = R + r
        nb = INF
        for a in [m["sampleAge"][p] if p < Kc else m["popAge"][p] for p in range(K)] + [x for b in range(B) for x in (m["bandStart"][b], m["bandEnd"][b])]:
            if a > t and a < nb:
                nb = a
        u = draw()
        w = -math.log(u) / R if R != 0.0 and R == R else INF
        jump = not (R > 0.0) or t + w >= nb
        tn = nb if jump else t + w
        if not tn < INF:
            return 2, None
        dt = tn - t
        for idx, _, c in rs:
            if idx < K:
                coalst[idx] = coalst[idx] + float(c * (c - 1)) * dt
            else:
                migst[idx - K] = migst[idx - K] + float(c) * dt
        t = tn
        if jump:
            enter(t)
            continue
        x = draw() * R
        acc, chosen = 0.0, -1
        for idx, r, _ in rs:
            acc = acc + r
            if chosen < 0 and x < acc:
                chosen = idx
        if chosen < 0:
            chosen = rs[-1][0]
        if chosen < K:
            p = chosen
            mine = [k for k, ln in enumerate(lin) if ln[1] == p]
            c = len(mine)
            a = min(int(draw() * float(c)), c - 1)
            b = min(int(draw() * float(c - 1)), c - 2)
            if b >= a:
                b += 1
            klo, khi = mine[min(a, b)], mine[max(a, b)]
            v = n + nco
            age[v], father[v], left[v], right[v], npop[v] = t, -1, lin[klo][0], lin[khi][0], p
            father[left[v]] = father[right[v]] = v
            lin[klo][0] = v
            del lin[khi]
            ncoal[p] += 1
            nco += 1
        else:
            b = chosen - K
            if len(migs) >= MAX_MIGS:
                return 1, None
            tgt, src = m["bandTgt"][b], m["bandSrc"][b]
            mine = [k for k, ln in enumerate(lin) if ln[1] == tgt]
            k = mine[min(int(draw() * float(len(mine))), len(mine) - 1)]
            migs.append((lin[k][0], b, src, tgt, t))
            lin[k][1] = src
            nmig[b] += 1
    return 2, None


def tree_length(age, father, root):
    ln = 0.0
    for v in range(len(age)):
        if v != root and 0 <= father[v] < len(age):
            ln = ln + (age[father[v]] - age[v])
    return ln


def gen_lnl(m, ncoal, coalst, nmig, migst):
    ln = 0.0
    for p in range(m["K"]):
        ln += float(ncoal[p]) * math.log(2 / m["theta"][p]) - coalst[p] / m["theta"][p]
    for b in range(m["B"]):
        if m["migRate"][b] > 0.0:
            ln += float(nmig[b]) * math.log(m["migRate"][b]) - migst[b] * m["migRate"][b]
    return ln


def simulate(m, seed, g, t):
    """the replicate of locus g at sample t: dict with `attempts` (those abandoned or failed before it), or None: failed"""
    for a in range(ATTEMPTS):
        st, rep = attempt(m, attempt_key(seed, g, t, a))
        if st == 0:
            rep["attempts"] = a
            rep["root"] = m["N"] - 1
            rep["genLnL"] = gen_lnl(m, rep["ncoal"], rep["coalst"], rep["nmig"], rep["migst"])
            rep["y"] = [rep["age"][rep["root"]], tree_length(rep["age"], rep["father"], rep["root"]), rep["genLnL"]] + \
                       [float(c) for c in rep["ncoal"]] + [float(c) for c in rep["nmig"]]
            return rep
    return None


def stat_names_gen(K, B):
    return ["tmrca", "length", "genLnL"] + [f"coal_{p}" for p in range(K)] + [f"mig_{b}" for b in range(B)]


def row_names(K, B, Kc, with_sites):
    s = stat_names_gen(K, B)[3:]
    return ["s." + x for x in s] + ["r." + x for x in s] + ["gt.tmrca", "gt.length", "gt.genLnL", "failed"] + (["r." + x for x in stat_names(Kc)] if with_sites else [])


# ---------------------------------------------------------------- the model of a chain's sample
def pack_model(pk, theta, popAge, sampleAge, migRate, bandStart, bandEnd):
    return make_model(pk.n, pk.Kc, pk.popFather, leaf_pops(pk), theta, popAge, sampleAge, pk.bandSrc, pk.bandTgt, migRate, bandStart, bandEnd)


def dumped_model(pk, path):
    """the model of the chain state as a state dump prints it (hex floats: exact)"""
    for ln in open(path):
        if ln.startswith("MODEL"):
            v = [float.fromhex(x) for x in ln.split()[1:]]
            K, B = pk.K, pk.B
            assert len(v) == 3 * (K + B)
            pops, bands = v[:3 * K], v[3 * K:]
            return pack_model(pk, pops[0::3], pops[1::3], pops[2::3], bands[0::3], bands[1::3], bands[2::3])
    raise AssertionError("no MODEL line in " + path)


def sampled_x(m, t, k, q):
    """the statistics of the sampled genealogy: gene-tree records t, sample k, record q"""
    n, N, K, B = m["n"], m["N"], m["K"], m["B"]
    age, father = [float(a) for a in t["age"][k, q]], [int(f) for f in t["father"][k, q]]
    root, nm = int(t["root"][k, q]), int(t["num_migs"][k, q])
    ncoal = [sum(1 for v in range(n, N) if int(t["npop"][k, q, v]) == p) for p in range(K)]
    nmig = [sum(1 for j in range(nm) if int(t["mig_band"][k, q, j]) == b) for b in range(B)]
    return [age[root], tree_length(age, father, root), float(t["genLnL"][k, q])] + [float(c) for c in ncoal] + [float(c) for c in nmig]


def model_loci(pk, models, t, rates, seed, S, loci, with_sites=True):
    """per locus of `loci` over the samples 0 .. S - 1 (models[k]: the chain's model at sample k; t: the chain's gene-tree records
    of the same loci): dict(acc [M][5], failed, site_acc [C][5], sites), the per-sample rows, the observed site row, and the
    replicates of the last sample"""
    n, K, B, Kc, pops = pk.n, pk.K, pk.B, pk.Kc, leaf_pops(pk)
    M, C = 3 + K + B, (1 + Kc * (Kc + 1) // 2) if with_sites else 0
    RC = 2 * (K + B) + 4
    out, rows, obs_row, last = [], [[0] * (RC + C) for _ in range(S)], [0] * C, []
    rec_loci = t["loci"].tolist()
    retried = 0
    for g in loci:
        q = rec_loci.index(g)
        acc, failed = [[0.0] * 5 for _ in range(M)], 0.0
        sacc, sites, missing = [], 0, None
        if with_sites:
            codes, counts = columns(pk, g)
            obs, sites = observed(pk, g)
            col = np.repeat(np.arange(len(counts)), counts)
            missing = (codes[col].T == 4) if sites else np.zeros((n, 0), bool)
            sacc = [[float(obs[c]), 0.0, 0.0, 0.0, 0.0] for c in range(C)]
            for c in range(C):
                obs_row[c] += obs[c]
        rep = None
        for k in range(S):
            m = models[k]
            rep = simulate(m, seed, g, k)
            if rep is None:
                failed = failed + 1.0
                rows[k][RC - 1] += 1
                continue
            retried += rep["attempts"] > 0
            x = sampled_x(m, t, k, q)
            for s in range(M):
                a, xv, yv = acc[s], x[s], rep["y"][s]
                if yv > xv:
                    a[0] = a[0] + 1.0
                    if s < 3:
                        rows[k][2 * (K + B) + s] += 1
                if yv == xv:
                    a[1] = a[1] + 1.0
                a[2] = a[2] + xv
                a[3] = a[3] + yv
                a[4] = a[4] + yv * yv
                if s >= 3:
                    rows[k][s - 3] += int(xv)
                    rows[k][K + B + s - 3] += int(yv)
            if with_sites:
                T = statistics(replicate(site_key(seed, g, k), rep["age"], rep["father"], float(rates[k, q]), n, sites), missing, pops, Kc)
                for c in range(C):
                    xv, a = float(T[c]), sacc[c]
                    if xv > a[0]:
                        a[1] = a[1] + 1.0
                    if xv == a[0]:
                        a[2] = a[2] + 1.0
                    a[3] = a[3] + xv
                    a[4] = a[4] + xv * xv
                    rows[k][RC + c] += T[c]
        out.append(dict(acc=acc, failed=failed, site_acc=sacc, sites=sites))
        last.append(rep)
    return out, rows, obs_row, last, retried


def f64_bits(x):
    return np.float64(x).view(np.uint64).item() if not isinstance(x, np.ndarray) else x.view(np.uint64)


def check_records(recs, last, m, what):
    """the decoded replicate records of the latest sample against the restatement, field by field; ages as bit patterns"""
    n, N = m["n"], m["N"]
    for q, rep in enumerate(last):
        if rep is None:
            assert int(recs["root"][q]) == -1 and int(recs["num_migs"][q]) == 0 and not recs["age"][q].any(), f"{what}: failed record {q}"
            assert not recs["records"][q][:16 * N].any()
            continue
        assert int(recs["root"][q]) == N - 1, f"{what}: record {q}: root"
        assert recs["age"][q].view(np.uint64).tolist() == np.array(rep["age"], np.float64).view(np.uint64).tolist(), f"{what}: record {q}: ages"
        for k in ("father", "left", "right", "npop"):
            assert recs[k][q].tolist() == rep[k], f"{what}: record {q}: {k}"
        assert recs["father"][q][N - 1] == -1 and sorted(recs["left"][q][n:].tolist() + recs["right"][q][n:].tolist()) == list(range(N - 1))
        nm = len(rep["migs"])
        assert nm <= MAX_MIGS and int(recs["num_migs"][q]) == nm, f"{what}: record {q}: migrations"
        for j, (br, band, sp, tp, ag) in enumerate(rep["migs"]):
            got = (int(recs["mig_branch"][q, j]), int(recs["mig_band"][q, j]), int(recs["mig_spop"][q, j]), int(recs["mig_tpop"][q, j]))
            assert got == (br, band, sp, tp) and float(recs["mig_age"][q, j]).hex() == ag.hex(), f"{what}: record {q}: migration {j}"
        assert float(recs["dataLnL"][q]) == 0.0 and float(recs["genLnL"][q]).hex() == rep["genLnL"].hex(), f"{what}: record {q}: genLnL"


def check_against_model(e, model, S, what, with_sites=True):
    Q, M = len(e["loci"]), len(e["stats"])
    assert e["samples"] == S and e["acc"].shape == (Q, M, 5) and len(model) == Q
    for q in range(Q):
        mo, g = model[q], int(e["loci"][q])
        assert float(e["failed"][q]) == mo["failed"], f"{what} S {S}: locus {g}: failed"
        for s in range(M):
            got, want = [float(v).hex() for v in e["acc"][q, s]], [float(v).hex() for v in mo["acc"][s]]
            assert got == want, f"{what} S {S}: locus {g} statistic {e['stats'][s]}: {e['acc'][q, s].tolist()} != {mo['acc'][s]}"
        if with_sites:
            assert int(e["sites"][q]) == mo["sites"]
            for c in range(len(e["site_stats"])):
                got, want = [float(v).hex() for v in e["site_acc"][q, c]], [float(v).hex() for v in mo["site_acc"][c]]
                assert got == want, f"{what} S {S}: locus {g} site statistic {e['site_stats'][c]}: {got} != {want}"
        else:
            assert e["site_acc"].size == 0


def check_rows(r, rows, obs_row, iters, what):
    its, got, obs = r["rows"]
    assert its.tolist() == list(range(iters)), what
    assert [int(v) for v in obs] == obs_row, f"{what}: the observed row"
    assert [[int(v) for v in row] for row in got] == rows, f"{what}: the per-sample rows"


# ---------------------------------------------------------------- one chain, sampled
GT_O_DATALNL = 3


def run_chain(lib, name, iters, tmp_path=None, seed=4242, loci=None, checkpoints=(), sample=True, trees=True, with_sites=True, record=None, final=None,
              pack=None, reset_at=None, set_model=None, iterate=True):
    """one chain over case `name` (lib None: the tightest capacity variant) with a sample of the gene trees, a dump of the model
    and a simulate sample after every iteration; Sampler.simulate() is fetched (no reset) after each of `checkpoints` samples and
    at the end, with the replicate records of that sample; the rows at the end.  set_model: a model (make_model) pushed into the
    engine after initialize; iterate False: the chain stands still (a hand-made model is not one the chain may run under)"""
    import gphocs_amd as G
    pk = pack or load_pack(name)
    s = G.Sampler(pk, lib=lib)
    try:
        if record:
            s.set_record_file(record)
        if sample:
            if trees:
                s.enable_gene_trees(iters, loci)
            s.simulate_enable(seed, iters, loci, with_sites=with_sites)
        s.initialize()
        if set_model is not None:
            push_model(s, set_model)
        hs0 = s.host_stats()
        at, recs, models = {}, {}, []
        for it in range(iters):
            if iterate:
                s.iteration(it)
            if sample:
                if trees:
                    s.sample_gene_trees(it)
                    if set_model is not None:
                        models.append(set_model)
                    else:
                        path = os.path.join(str(tmp_path), f"{name}.{it}.model")
                        s.dump_state(path, False)
                        models.append(dumped_model(pk, path))
                        os.unlink(path)
                if reset_at == it:
                    s.simulate(reset=True)
                s.simulate_sample(it)
                if it + 1 in checkpoints:
                    at[it + 1], recs[it + 1] = s.simulate(), s.simulate_records(raw=True)
        hs1 = s.host_stats()
        launches = s.class_stats(CLS)["launches"]
        s.set_record_file(None)
        rows = None
        if sample:
            at[iters], recs[iters] = s.simulate(), s.simulate_records(raw=True)
            rows = s.simulate_rows()
        t = rates = None
        if sample and trees:
            off = s._gene_trees_shape()[3][GT_O_DATALNL]
            t = s.gene_trees(raw=True)
            rec = t["records"]
            rates = np.ascontiguousarray(rec[:, :, off + 32:off + 40]).view(np.float64)[:, :, 0] if rec.size else np.zeros(rec.shape[:2])
        if final:
            s.dump_state(final, True)
        return dict(si=at, recs=recs, rows=rows, trees=t, rates=rates, models=models, pack=pk, stats=(hs0, hs1), launches=launches, oob=s.debug_oob(),
                    seed=seed, columns=(s.simulate_columns(0), s.simulate_columns(1), s.simulate_columns(2)) if sample else None)
    finally:
        s.close()


def push_model(s, m):
    """a hand-made model into the engine's chain state (gph_engine_set_model; pushed to the device before the next sample)"""
    def arr(v):
        a = np.ascontiguousarray(list(v) + [0.0], dtype=np.float64)
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert (m["n"], m["K"], m["Kc"], m["B"]) == (s.pack.n, s.pack.K, s.pack.Kc, s.pack.B) and m["bandSrc"] == s.pack.bandSrc.tolist()
    assert m["bandTgt"] == s.pack.bandTgt.tolist() and m["popFather"] == s.pack.popFather.tolist()
    keep = [arr(m[k]) for k in ("theta", "popAge", "sampleAge", "migRate", "bandStart", "bandEnd")]
    assert s.lib.gph_engine_set_model(s.engine, *[p for _, p in keep]) == 0


def check_case(lib, name, tmp_path, iters=9, checkpoints=CHECKPOINTS, loci=None, key="cpu", pack=None, with_sites=True, set_model=None, iterate=True,
               seed=4242):
    """bit for bit: every fetch at the checkpoints against the restatement over the chain's own records and models"""
    r = run_chain(lib, name, iters, tmp_path, seed=seed, loci=loci, checkpoints=[c for c in checkpoints if c < iters], pack=pack, with_sites=with_sites,
                  set_model=set_model, iterate=iterate)
    pk, t = r["pack"], r["trees"]
    sel = list(range(pk.L)) if loci is None else list(loci)
    assert r["launches"] == iters and r["oob"][0] == 0
    assert t["loci"].tolist() == sel
    assert r["columns"][0] == stat_names_gen(pk.K, pk.B) and r["columns"][1] == row_names(pk.K, pk.B, pk.Kc, with_sites)
    assert r["columns"][2] == (stat_names(pk.Kc) if with_sites else [])
    for S, e in sorted(r["si"].items()):
        assert e["loci"].tolist() == sel
        model, rows, obs_row, last, retried = model_loci(pk, r["models"], t, r["rates"], r["seed"], S, sel, with_sites)
        check_against_model(e, model, S, name, with_sites)
        check_records(r["recs"][S], last, r["models"][S - 1], f"{name} S {S}")
    check_rows(r, rows, obs_row, iters, name)
    migs = sum(len(rep["migs"]) for rep in last if rep)
    failed = sum(m["failed"] for m in model)
    print(f"{name} [{key}] n {pk.n} K {pk.K} B {pk.B} loci {len(model)} samples {iters}: last sample: {migs} migrations, retried {retried}, "
          f"failed {failed:g}, last row {rows[-1]}")
    r["model"], r["last"], r["retried"] = model, last, retried
    return r


# ---------------------------------------------------------------- the restatement pinned by analysis
def closed_form_model_1():
    """A and B with two haploid leaves each, no band: (model, tau, thetas)"""
    tau, thA, thB, thR = 0.01, 0.03, 0.025, 0.02
    return make_model(4, 2, [2, 2, -1], [0, 0, 1, 1], [thA, thB, thR], [0.0, 0.0, tau], [0.0, 0.0, 0.0]), tau, (thA, thB, thR)


def closed_form_model_2():
    """one leaf each, one band B -> A (target A: a lineage in A moves, backwards, to B) live on [0, tau)"""
    tau, thB, mr = 0.01, 0.03, 70.0
    return make_model(2, 2, [2, 2, -1], [0, 1], [0.02, thB, 0.02], [0.0, 0.0, tau], [0.0, 0.0, 0.0], [1], [0], [mr], [0.0], [tau]), tau, thB, mr


# ---------------------------------------------------------------- hand-made models on the 4-leaf pack
def edge_models():
    """name -> model on the 4-leaf pack (A: leaves 0, 1; B: leaves 2, 3; root 2).  Bands are given by hand, so a band may
    start after 0 and end before tau"""
    tau = 0.02
    base = dict(n=4, Kc=2, popFather=[2, 2, -1], leafpop=[0, 0, 1, 1], theta=[0.05, 0.04, 0.03], popAge=[0.0, 0.0, tau])
    two = dict(bandSrc=[1, 0], bandTgt=[0, 1])

    def mk(sampleAge, rates, starts, ends):
        return make_model(sampleAge=sampleAge, migRate=rates, bandStart=starts, bandEnd=ends, **base, **two)
    return {
        # retries: rates at which some attempts pass 10 migrations and most do not
        "cap": mk([0.0, 0.0, 0.0], [150.0, 150.0], [0.0, 0.0], [tau, tau]),
        # every attempt passes the cap: 4 lineages x 1e6 x tau = 8e4 expected migrations
        "all-fail": mk([0.0, 0.0, 0.0], [1e6, 1e6], [0.0, 0.0], [tau, tau]),
        # a band that starts after 0 and ends before its populations' father; the other is never live
        "inner-band": mk([0.0, 0.0, 0.0], [400.0, 0.0], [0.004, 0.0], [0.012, 0.0]),
        # B's samples enter at 0.008, above the start of a band into B; a band into A
        "late-samples": mk([0.0, 0.008, 0.0], [200.0, 300.0], [0.002, 0.003], [tau, 0.015]),
        # boundaries that share an age: B enters where one band starts and the other ends; a band ends at tau
        "shared-ages": mk([0.0, 0.006, 0.0], [250.0, 250.0], [0.006, 0.001], [tau, 0.006]),
    }


EDGE_BANDS = """MIG-BANDS-START
	BAND-START
		source	B
		target	A
		mig-rate-print	0.1
	BAND-END
	BAND-START
		source	A
		target	B
		mig-rate-print	0.1
	BAND-END
MIG-BANDS-END
"""


def edge_model_bands(tmp_path, lib):
    """predictive_util.edge_model's pack (4 leaves, A and B) with a band in each direction: band 0 into A, band 1 into B"""
    import gphocs_amd as G
    from predictive_util import EDGE_CTL, EDGE_SEQ
    d = tmp_path / "edge-bands"
    os.makedirs(d, exist_ok=True)
    (d / "e.ctl").write_text(EDGE_CTL + EDGE_BANDS)
    (d / "e.seq").write_text(EDGE_SEQ)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        p = G.Pack.from_control("e.ctl", lib=lib)
    finally:
        os.chdir(cwd)
    assert (p.n, p.Kc, p.K, p.B) == (4, 2, 3, 2) and p.bandSrc.tolist() == [1, 0] and p.bandTgt.tolist() == [0, 1]
    return p


def check_edge_model(lib, base, tmp_path, which, iters=24, with_sites=True):
    from predictive_util import edge_pack
    pk = edge_pack(base, [[("AACC", 30), ("ACGT", 20), ("ANCA", 7)], [("ACCA", 1)], [("AAAC", 200), ("ACAC", 50)]])
    m = edge_models()[which]
    return check_case(lib, which, tmp_path, iters=iters, checkpoints=(1, 2), pack=pk, set_model=m, iterate=False, with_sites=with_sites, seed=99), m


# ---------------------------------------------------------------- seed, selections, lifecycle, sites off, the chain untouched
def check_seed(lib, tmp_path, name="m3", iters=3):
    a = run_chain(lib, name, iters, tmp_path, seed=1, trees=False)
    b = run_chain(lib, name, iters, tmp_path, seed=2, trees=False)
    c = run_chain(lib, name, iters, tmp_path, seed=1, trees=False)
    ea, eb, ec = a["si"][iters], b["si"][iters], c["si"][iters]
    assert ea["acc"].tobytes() == ec["acc"].tobytes() and ea["site_acc"].tobytes() == ec["site_acc"].tobytes()
    assert a["rows"][1].tobytes() == c["rows"][1].tobytes() and a["recs"][iters]["records"].tobytes() == c["recs"][iters]["records"].tobytes()
    assert ea["acc"][:, :, 3].tolist() != eb["acc"][:, :, 3].tolist()                  # sy moves with the seed
    assert ea["acc"][:, :, 2].tolist() == eb["acc"][:, :, 2].tolist()                  # sx, the sampled genealogy, does not
    assert ea["site_acc"][:, :, 0].tolist() == eb["site_acc"][:, :, 0].tolist()
    assert a["recs"][iters]["records"].tobytes() != b["recs"][iters]["records"].tobytes()
    big = check_case(lib, name, tmp_path, iters=1, checkpoints=(), seed=(1 << 64) - 3)         # a seed that uses all 64 bits
    assert big["si"][1]["samples"] == 1


def check_selections(lib, tmp_path, name="m3", iters=4):
    """a stride and the last locus alone: each row of the selection equals the same locus's row of the all-loci run (the key holds
    the GLOBAL locus index); the usage errors; a rank without a selected locus"""
    import gphocs_amd as G
    everything = check_case(lib, name, tmp_path, iters=iters, checkpoints=())
    pk = everything["pack"]
    L = pk.L
    full = everything["si"][iters]
    for sel in ([0, 2, 4], [L - 1]):
        r = check_case(lib, name, tmp_path, iters=iters, checkpoints=(), loci=sel)
        e = r["si"][iters]
        assert e["acc"].tobytes() == full["acc"][sel].tobytes() and e["site_acc"].tobytes() == full["site_acc"][sel].tobytes()
        assert r["recs"][iters]["records"].tobytes() == everything["recs"][iters]["records"][sel].tobytes()
    s = G.Sampler(pk, lib=lib)
    try:
        for bad in ([3, 2], [2, 2], [-1], [0, -1]):
            with pytest.raises(ValueError):
                s.simulate_enable(1, 4, bad)
            assert s.lib.gph_engine_simulate_enable(s.engine, 1, 4, (ctypes.c_int64 * len(bad))(*bad), len(bad), 1, 0) == EARG
        assert s.lib.gph_engine_simulate_enable(s.engine, 1, -1, None, 0, 1, 0) == EARG
        s.simulate_enable(1, 4, [L + 5])       # beyond the rank's block: ignored -- the rank takes its (zero) rows and launches nothing
        s.initialize()
        n0 = s.host_stats()["launches"]
        s.simulate_sample(0)
        s.simulate_sample(1)
        assert s.host_stats()["launches"] == n0 and s.class_stats(CLS)["launches"] == 0
        e = s.simulate()
        assert e["samples"] == 2 and e["loci"].tolist() == [] and e["acc"].shape == (0, 3 + pk.K + pk.B, 5)
        its, rows, obs = s.simulate_rows()
        assert its.tolist() == [0, 1] and not rows.any() and not obs.any()
        assert s.simulate_records()["root"].shape == (0,)
    finally:
        s.close()


def check_lifecycle(lib, G, name="m3", iters=3):
    """reset (accumulators zeroed, obs formed again, t back at 0), enable twice, a full row buffer, GPH_EFULL with nothing
    allocated, GPH_ESTATE -- as for the predictive checks"""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    L, K, B, Kc, cap = pk.L, pk.K, pk.B, pk.Kc, 2 * iters
    M, C, N = 3 + K + B, 1 + Kc * (Kc + 1) // 2, 2 * pk.n - 1
    RC = 2 * (K + B) + 4 + C
    s = G.Sampler(pk, lib=lib)
    try:
        with pytest.raises(RuntimeError):
            s.simulate()                                    # not enabled
        assert s.lib.gph_engine_simulate_fetch_loci(s.engine, None, None, None, 0) == ESTATE
        assert s.lib.gph_engine_simulate_sample(s.engine, 0) == ESTATE
        assert s.lib.gph_engine_simulate_fetch_records(s.engine, None, None) == ESTATE
        assert s._simulate_shape() == (0, 0, 0, 0, 0, 0, 0)
        s.simulate_enable(7, cap)
        Q, m_, c_, rc_, rb, S_, held = s._simulate_shape()
        assert (Q, m_, c_, rc_, S_, held) == (L, M, C, RC, 0, 0) and rb >= 16 * N + 8 * 10 + 12 * 10 + 2 * 10 + 16
        need = ((L * (5 * M + 1) * 8 + L * C * 40 + C * 8 + 2 * L * 8 + pk.n + 15) & ~15) + L * rb + cap * RC * 8
        assert s.lib.gph_engine_simulate_sample(s.engine, 0) == ESTATE           # before initialize
        assert s.lib.gph_engine_simulate_enable(s.engine, 7, cap, None, 0, 1, need - 1) == FULL
        assert s._simulate_shape() == (0, 0, 0, 0, 0, 0, 0)  # nothing allocated, the feature is off
        with pytest.raises(MemoryError):
            s.simulate_enable(7, cap, max_bytes=need - 1)
        s.initialize()                                      # the engine is still usable
        with pytest.raises(RuntimeError):
            s.simulate_sample(0)
        s.simulate_enable(7, cap, [1, 2])                   # enable twice: another selection, then the real one
        assert s._simulate_shape()[:4] == (2, M, C, RC)
        s.simulate_enable(7, cap, max_bytes=need)
        want_obs = [observed(pk, g)[0] for g in range(L)]
        before = s.simulate()
        assert before["samples"] == 0 and not before["acc"].any() and not before["failed"].any()
        assert before["site_acc"][:, :, 0].astype(np.int64).tolist() == want_obs and not before["site_acc"][:, :, 1:].any()
        assert (s.simulate_records()["root"] == 0).all() and not s.simulate_records(raw=True)["records"].any()   # no sample yet: zeros
        for it in range(iters):
            s.iteration(it)
            s.simulate_sample(it)
        first = s.simulate(reset=True)
        assert first["samples"] == iters and first["acc"][:, :, 3].any()
        zero = s.simulate()
        assert zero["samples"] == 0 and zero["acc"].tobytes() == before["acc"].tobytes() and zero["site_acc"].tobytes() == before["site_acc"].tobytes()
        for it in range(iters, 2 * iters):
            s.iteration(it)
            s.simulate_sample(it)
        assert s._simulate_shape()[5:] == (iters, cap)
        with pytest.raises(BufferError):
            s.simulate_sample(99)                           # the row buffer is full
        second = s.simulate()
        its, rows, obs = s.simulate_rows()
        assert its.tolist() == list(range(2 * iters)) and s._simulate_shape()[6] == 0
        assert [int(v) for v in obs] == [sum(o[c] for o in want_obs) for c in range(C)]
        s2 = G.Sampler(pk, lib=lib)                         # the same chain, sampled over the second half only: t restarts at 0
        try:
            s2.initialize()
            for it in range(2 * iters):
                if it == iters:
                    s2.simulate_enable(7, cap)
                s2.iteration(it)
                if it >= iters:
                    s2.simulate_sample(it)
            fresh = s2.simulate()
            rows2 = s2.simulate_rows()[1]
        finally:
            s2.close()
        assert second["samples"] == fresh["samples"] == iters
        assert second["acc"].tobytes() == fresh["acc"].tobytes() != first["acc"].tobytes()
        assert second["site_acc"].tobytes() == fresh["site_acc"].tobytes()
        assert rows[iters:].tobytes() == rows2.tobytes()
        s.initialize()                                      # a new chain starts from zeroed accumulators and no rows
        again = s.simulate()
        assert again["samples"] == 0 and again["acc"].tobytes() == before["acc"].tobytes() and s._simulate_shape()[6] == 0
        s.simulate_enable(7, 0)                             # capacity 0: off
        assert s._simulate_shape() == (0, 0, 0, 0, 0, 0, 0)
    finally:
        s.close()


def check_refused_locus(lib, base, capfd):
    """sites x max n_p n_q = 2^32: refused by name with sites, taken without"""
    import gphocs_amd as G
    from predictive_util import edge_pack
    count = (1 << 32) // 4
    pk = edge_pack(base, [[("AACC", 5)], [("AACC", count // 2), ("ACCA", count - count // 2)]])
    s = G.Sampler(pk, lib=lib)
    try:
        capfd.readouterr()
        rc = s.lib.gph_engine_simulate_enable(s.engine, 1, 4, None, 0, 1, 0)
        err = capfd.readouterr().err
        assert rc == EARG and "locus 1" in err and "2^32" in err, err
        assert s._simulate_shape() == (0, 0, 0, 0, 0, 0, 0)
        with pytest.raises(ValueError):
            s.simulate_enable(1, 4)
        s.simulate_enable(1, 4, with_sites=False)           # the genealogy level has no such bound
        assert s._simulate_shape()[:3] == (2, 3 + pk.K + pk.B, 0)
        s.simulate_enable(1, 4, [0])
        assert s._simulate_shape()[0] == 1
    finally:
        s.close()


def check_sites_off(lib, tmp_path, name="m3", iters=3):
    """with_sites = 0 leaves the genealogy-level words, the records and the genealogy columns of the rows identical"""
    on = run_chain(lib, name, iters, tmp_path, trees=False)
    off = run_chain(lib, name, iters, tmp_path, trees=False, with_sites=False)
    a, b = on["si"][iters], off["si"][iters]
    assert a["acc"].tobytes() == b["acc"].tobytes() and a["failed"].tobytes() == b["failed"].tobytes()
    assert on["recs"][iters]["records"].tobytes() == off["recs"][iters]["records"].tobytes()
    wide = off["rows"][1].shape[1]
    assert wide == 2 * (on["pack"].K + on["pack"].B) + 4 and on["rows"][1][:, :wide].tobytes() == off["rows"][1].tobytes()
    assert b["site_acc"].size == 0 and b["site_stats"] == [] and off["rows"][2].size == 0
    assert off["launches"] == on["launches"] == iters


def check_chain_untouched(lib, name, full, tmp_path, tol=1e-12, predictive=False):
    """records and final state dump with sampling on identical to a run with sampling off, and still the reference's records;
    launches of class 25 = the samples.  predictive: --predictive's sampler runs next to it in both runs, and its accumulators
    and rows are the same bytes"""
    import gphocs_amd as G
    out = []
    for on in (True, False):
        rec, final = str(tmp_path / f"{name}.{int(on)}.rtrace"), str(tmp_path / f"{name}.{int(on)}.final")
        pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        s = G.Sampler(pk, lib=lib)
        try:
            s.set_record_file(rec)
            if on:
                s.simulate_enable(4242, full)
            if predictive:
                s.predictive_enable(4242, full)
            s.initialize()
            hs0 = s.host_stats()
            for it in range(full):
                s.iteration(it)
                if on:
                    s.simulate_sample(it)
                if predictive:
                    s.predictive_sample(it)
            hs1 = s.host_stats()
            launches = s.class_stats(CLS)["launches"]
            s.set_record_file(None)
            pd = (s.predictive()["acc"].tobytes(), s.predictive_rows()[1].tobytes()) if predictive else None
            samples = s.simulate()["samples"] if on else 0
            s.dump_state(final, True)
            out.append(dict(rec=rec, final=final, stats=(hs0, hs1), launches=launches, samples=samples, pd=pd))
        finally:
            s.close()
    on, off = out
    assert open(on["rec"]).read() == open(off["rec"]).read()
    assert open(on["final"]).read() == open(off["final"]).read()
    assert compare_records(on["rec"], os.path.join(GOLDEN, name + ".rtrace")) <= tol
    assert on["samples"] == full and on["launches"] == full and off["launches"] == 0
    assert on["pd"] == off["pd"]
    return on, off


# ---------------------------------------------------------------- the program and the launcher
def _g(x):
    return "%.10g" % x


def api_files(ctl_dir, ctl, spec_loci, seed=None, lib=None, sampler_lib=None, with_sites=True):
    """the text of PREFIX.simulate.tsv and PREFIX.simulate-genome.tsv the program must write, formatted here from the API's values
    of an equivalent Sampler run (burn-in first) that samples wherever a trace line is written (the API's values themselves are
    what the bit-for-bit tests hold to the restatement)"""
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(ctl_dir)
    try:
        p = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    sel = list(range(p.L)) if spec_loci is None else list(spec_loci)
    seed = p.seed if seed is None else seed
    its = [it for it in range(p.numSamplesMcmc) if it % (p.sampleSkip + 1) == 0]
    s = G.Sampler(p, lib=sampler_lib)
    try:
        s.simulate_enable(seed & M64, len(its), sel, with_sites=with_sites)
        s.initialize()
        for it in range(-p.burnin, p.numSamplesMcmc):
            s.iteration(it)
            if it in its:
                s.simulate_sample(it)
        e = s.simulate()
        _, rows, obs_row = s.simulate_rows()
    finally:
        s.close()
    S, K, B, Kc = len(its), p.K, p.B, p.Kc
    bands = [f"{p.popName[int(a)]}->{p.popName[int(b)]}" for a, b in zip(p.bandSrc, p.bandTgt)]
    names = ["tmrca", "length", "genLnL"] + [f"coal_{p.popName[k]}" for k in range(K)] + [f"mig_{b}" for b in bands]
    snames = (["seg"] + [f"diff_{p.popName[a]}|{p.popName[b]}" for a in range(Kc) for b in range(a, Kc)]) if with_sites else []
    M, C = len(names), len(snames)
    head = ["locus", "name", "samples", "failed", "sites"] + [f"{k}_{nm}" for nm in names for k in ("s", "mean", "sd", "p")] + \
           [f"{k}_{nm}" for nm in snames for k in ("obs", "mean", "sd", "p")] + ["minP", "stat"]
    out, lowest, failed_all = ["\t".join(head)], None, 0
    for q, g in enumerate(sel):
        failed = float(e["failed"][q])
        n = float(S) - failed
        failed_all += int(failed)
        cells, minp, at = [], None, None
        for c in range(M + C):
            if c < M:
                gt, eq, sx, s1, s2 = [float(v) for v in e["acc"][q, c]]
                first = sx / n if n > 0 else 0.0
            else:
                first, gt, eq, s1, s2 = [float(v) for v in e["site_acc"][q, c - M]]
            mean = s1 / n if n > 0 else 0.0
            var = (s2 - s1 * s1 / n) / (n - 1) if n > 1 else 0.0
            pv = (gt + eq / 2) / n if n > 0 else 0.0
            two = 2 * min(pv, 1 - pv)
            if minp is None or two < minp:
                minp, at = two, c
            cells += [_g(first), _g(mean), _g(math.sqrt(var) if var > 0.0 else 0.0), _g(pv)]
        if failed < S and (lowest is None or minp < lowest[0]):
            lowest = (minp, g)
        out.append("\t".join([str(g), p.locusNames[g], str(S), str(int(failed)), str(int(e["sites"][q]))] + cells + [_g(minp), (names + snames)[at]]))
    lowest = lowest or (0.0, -1)
    out.append("# loci %d samples %d seed %d failed %d minMinP %s (locus %d)" % (len(sel), S, seed & M64, failed_all, _g(lowest[0]), lowest[1]))
    KB = K + B
    cols = ["s." + x for x in names[3:]] + ["r." + x for x in names[3:]] + ["gt." + x for x in names[:3]] + ["failed"] + ["r." + x for x in snames]
    W = len(cols)
    rows = [[int(v) for v in r] for r in rows]
    assert all(len(r) == W for r in rows) and len(rows) == S
    gen = ["\t".join(["iter"] + cols)] + ["%7d" % it + "".join("\t%d" % v for v in rows[k]) for k, it in enumerate(its)]
    live = sum(len(sel) - r[2 * KB + 3] for r in rows)
    obs, mean, pl = "# observed", "# mean", "# p"
    for c in range(W):
        site, rep = c > 2 * KB + 3, KB <= c < 2 * KB
        col = [r[c] for r in rows]
        against = [int(obs_row[c - 2 * KB - 4])] * S if site else [r[c - KB] for r in rows] if rep else [0] * S
        obs += "\t%d" % against[0] if site else "\t-"
        mean += "\t" + _g(float(sum(col)) / float(S))
        if site or rep:
            pl += "\t" + _g((sum(v > a for v, a in zip(col, against)) + sum(v == a for v, a in zip(col, against)) / 2) / float(S))
        elif 2 * KB <= c < 2 * KB + 3:
            pl += "\t" + _g(float(sum(col)) / float(live) if live > 0 else 0.0)
        else:
            pl += "\t-"
    gen += [obs, mean, pl, "# loci %d samples %d seed %d" % (len(sel), S, seed & M64)]
    return "\n".join(out) + "\n", "\n".join(gen) + "\n", "Simulate: " + pl[2:]


def check_program(lib_path, lib, tmp_path):
    """both files hold the API's values, character for character, and the log repeats the p line; --simulate-seed, --simulate-rows
    (a buffer that fills several times) and --simulate-no-sites; the trace and --predictive's files do not move; with --mc3 (no
    swaps) and --replicates the files are chain 0's = the plain run's; the usage errors"""
    import subprocess
    import gphocs_amd as G
    from sampler_util import EXE, _copy_case, _run, read_outputs
    from test_gene_trees import PROGRAM_CASE, PROGRAM_LOCI, PROGRAM_SPEC, program_ctl
    name = PROGRAM_CASE
    ctl = name + ".ctl"
    a, b, c, d, e, m, r = (tmp_path / x for x in ("with", "without", "seed", "all", "rest", "mc3", "rep"))
    for x in (a, b, c, d, e, m, r):
        _copy_case(name, x, program_ctl(name))
    on = ["--simulate", "out", "--simulate-loci", PROGRAM_SPEC]
    run = _run(lib_path, a, on + [ctl])
    _run(lib_path, b, [ctl])
    trace = a / (name + ".trace")
    assert open(trace).read() == open(b / (name + ".trace")).read()
    assert not read_outputs(b, "out")
    got = read_outputs(a, "out")
    assert sorted(got) == ["simulate-genome.tsv", "simulate.tsv"]                # no part left behind
    want_loci, want_genome, want_log = api_files(str(a), ctl, PROGRAM_LOCI, None, lib, lib)
    assert got["simulate.tsv"] == want_loci
    assert got["simulate-genome.tsv"] == want_genome
    assert want_log in run.stdout.splitlines()
    head = got["simulate.tsv"].splitlines()[0].split("\t")
    assert head[:9] == ["locus", "name", "samples", "failed", "sites", "s_tmrca", "mean_tmrca", "sd_tmrca", "p_tmrca"] and head[-2:] == ["minP", "stat"]
    # another seed, a row buffer of 3 rows that fills several times, all loci, no sites
    _run(lib_path, c, ["--simulate", "out", "--simulate-seed", "18446744073709551614", "--simulate-rows", "3", "--simulate-no-sites", ctl])
    other = read_outputs(c, "out")
    want_loci2, want_genome2, _ = api_files(str(c), ctl, None, (1 << 64) - 2, lib, lib, with_sites=False)
    assert other["simulate.tsv"] == want_loci2 and other["simulate-genome.tsv"] == want_genome2
    assert "obs_seg" not in want_loci2 and "obs_seg" in want_loci
    # --predictive next to it writes the same bytes as alone; the trace does not move
    _run(lib_path, d, on + ["--predictive", "pp", "--gene-trees", "gt", "--gene-trees-loci", "1-5", ctl])
    _run(lib_path, e, ["--predictive", "pp", "--gene-trees", "gt", "--gene-trees-loci", "1-5", ctl])
    assert read_outputs(d, "out") == got
    for prefix, count in (("pp", 2), ("gt", 1)):
        others = read_outputs(e, prefix)
        assert len(others) == count and read_outputs(d, prefix) == others
    assert open(d / (name + ".trace")).read() == open(e / (name + ".trace")).read() == open(trace).read()
    # chain 0 of a group of chains is the plain run's chain
    _run(lib_path, m, ["--mc3", "2", "--mc3-swap-every", "-1"] + on + [ctl])
    assert read_outputs(m, "out") == got
    _run(lib_path, r, ["--replicates", "2", "--replicates-out", "rep"] + on + [ctl])
    assert read_outputs(r, "out") == got
    # usage errors: they name the option, before anything is read, nothing written
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    u = tmp_path / "usage"
    _copy_case(name, u, program_ctl(name))
    L = G.Pack.load(os.path.join(GOLDEN, name + ".gpk")).L
    pre = ["--simulate", "out"]
    for args, words in ((["--simulate-loci", "0-3"], ["--simulate "]), (["--simulate-seed", "5"], ["--simulate "]), (["--simulate-rows", "4"], ["--simulate "]),
                        (["--simulate-no-sites"], ["--simulate "]),
                        (pre + ["--simulate-loci", "0-4,3"], ["locus 3 ", "--simulate-loci"]), (pre + ["--simulate-loci", "5,5"], ["locus 5 ", "--simulate-loci"]),
                        (pre + ["--simulate-loci", f"3,{L}"], [f"locus {L} ", "--simulate-loci"]), (pre + ["--simulate-loci", "2-x"], ["2-x", "--simulate-loci"]),
                        (pre + ["--simulate-seed", "-4"], ["--simulate-seed"]), (pre + ["--simulate-seed", "7x"], ["--simulate-seed"]),
                        (pre + ["--simulate-rows", "0"], ["usage"])):
        res = subprocess.run([EXE] + args + [ctl], cwd=u, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode != 0 and all(w in res.stderr for w in words), (args, res.stderr[-500:])
        assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"]), args
    cwd = os.getcwd()
    os.chdir(u)
    try:
        p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
        anylib = lib or G.load_library(dims=(p.n, p.K, p.B))
        for kw in (dict(simulate_loci="0-3"), dict(simulate_seed=5), dict(simulate_rows=4), dict(simulate_no_sites=True), dict(simulate="out", simulate_rows=-1)):
            assert G.run_control_file(anylib, ctl, **kw) == EARG
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(u)) == sorted([ctl, name + ".seq"])


def check_ranks(lib_path, lib, tmp_path, name="m3"):
    """two shared-memory ranks' parts, joined by gph_simulate_write, are the one-rank files -- per-locus rows concatenated, per-sample
    rows added (the key holds the global locus index) -- for all loci and for a selection that lies wholly in rank 1's block; the
    launcher does the same; a part cut short is refused and nothing is left"""
    import shutil
    from sampler_util import _copy_case, _run, read_outputs, run_ranks
    for tag, spec in (("all", None), ("upper", "9-15:2")):
        one, two, three = tmp_path / f"one-{tag}", tmp_path / f"two-{tag}", tmp_path / f"g2-{tag}"
        pk = run_ranks(lib_path, name, 1, one, simulate="out", simulate_loci=spec)
        want = read_outputs(one, "out")
        assert sorted(want) == ["simulate-genome.tsv", "simulate.tsv"]
        loci = list(range(pk.L)) if spec is None else [9, 11, 13, 15]
        assert [int(ln.split("\t")[0]) for ln in want["simulate.tsv"].splitlines()[1:-1]] == loci
        run_ranks(lib_path, name, 2, two, simulate="out", simulate_loci=spec)
        assert sorted(f for f in os.listdir(two) if f.startswith("out.")) == ["out.simulate.part0", "out.simulate.part1"]
        if spec is None:
            cut = tmp_path / "cut"
            os.makedirs(cut)
            for r in range(2):
                shutil.copy(two / f"out.simulate.part{r}", cut)
            text = open(cut / "out.simulate.part1").read().splitlines(True)
            open(cut / "out.simulate.part1", "w").write("".join(text[:-1]))
            assert lib.gph_simulate_write(str(cut / "out").encode(), 2) != 0
            assert not read_outputs(cut, "out")
        assert lib.gph_simulate_write(str(two / "out").encode(), 2) == 0
        assert read_outputs(two, "out") == want                          # no part among them
        if spec is not None:
            _copy_case(name, three)
            _run(lib_path, three, ["-g", "2", "--simulate", "out", "--simulate-loci", spec, name + ".ctl"])
            assert read_outputs(three, "out") == want


def check_failed_runs_leave_nothing(lib_path, tmp_path):
    """a run made to fail late -- the chain has run to its end, a directory sits where PREFIX.simulate-genome.tsv must be written:
    status non-zero, no part and no file of ours left, for one rank and for two"""
    import subprocess
    from sampler_util import EXE, _copy_case
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    for ranks in (1, 2):
        d = tmp_path / f"f{ranks}"
        _copy_case("m3", d)
        os.mkdir(d / "out.simulate-genome.tsv")
        args = (["-g", str(ranks)] if ranks > 1 else []) + ["--simulate", "out", "m3.ctl"]
        r = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0
        assert len(open(d / "m3.trace").read().splitlines()) == 121        # the chain itself ran to its end
        assert [f for f in os.listdir(d) if f.startswith("out.")] == ["out.simulate-genome.tsv"] and not os.listdir(d / "out.simulate-genome.tsv")
