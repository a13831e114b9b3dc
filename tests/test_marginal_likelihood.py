"""`G-PhoCS-hip --beta B` and `--marginal-likelihood PREFIX` on the CPU (the host build of the engine sources).

F  the two estimates of ln Z against a number computed independently.  The model of power_posterior_util.py (two populations,
   one haploid sample each, six loci of 200 sites with 0 .. 12 differences) has ln Z as a three-dimensional integral, written
   there in numpy from the model's definition; the formulas are first held against the engine's own genLnL and dataLnL at a
   state of the chain, to 1e-10.  The ladder runs through gph_run with K = 16, b = 100, s = 400 (3 s on the host build).
   The tolerance is 4 standard deviations of the estimate over 8 seeds plus the quadrature's refinement error, from these runs
   of the same sizes on the host build (seeds 101 .. 108 of the control file):
     lnZ_ss  -1834.512918 -1834.901761 -1834.428529 -1834.319759 -1834.467412 -1834.442807 -1835.373523 -1834.784350
             mean -1834.6539, standard deviation 0.3501
     lnZ_ti  -1834.652895 -1834.850227 -1834.414552 -1834.270862 -1834.479089 -1834.528134 -1835.220768 -1834.878050
             mean -1834.6618, standard deviation 0.3071
     quadrature  -1834.6749557 at steps (1e-4, 2e-4), -1834.6744473 at (2e-4, 4e-4): refinement error 5.1e-4 (the test
             recomputes both)
     tolerance   lnZ_ss 4 x 0.3501 + 5.1e-4 = 1.4009,  lnZ_ti 4 x 0.3071 + 5.1e-4 = 1.2289
   On a pack with no information (every base N) both estimates are exactly 0.
G  the program: trace and -l file byte-identical with and without the ladder, K + 1 rows with the formula's beta, the `#`
   line against the estimates recomputed in numpy from the per-rung series of a Sampler stepped down the same ladder by hand
   (same seed, same bits), the usage errors, and no file after a failed run.
H  --beta 1 leaves the trace as it is; --beta 0.5 on a sequence file whose alignments are concatenated with themselves gives
   the parameter columns of the plain run character for character."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from sampler_util import EXE, _copy_case, hostemu_library
import power_posterior_util as U

SD_SS, SD_TI = 0.3501, 0.3071       # over the 8 seeds of the docstring
ML = dict(K=16, b=100, s=400)


@pytest.fixture(scope="module")
def hostemu():
    return hostemu_library()


def program(hostemu_path, cwd, args, ok=True):
    env = dict(os.environ, GPHOCS_HIP_LIB=hostemu_path) if hostemu_path else dict(os.environ)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def read_table(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == "rung beta samples meanLnL sdLnL lnRatio accCoal accMig accSpr accTheta accMigRate accTau accMixing".split()
    rows = [[float(x) for x in ln.split("\t")] for ln in lines[1:-1]]
    t = lines[-1].split()
    assert t[0] == "#" and t[1] == "lnZ_ss" and t[3] == "lnZ_ti" and t[5] == "steps" and t[7] == "alpha"
    return rows, float(t[2]), float(t[4]), int(t[6]), float(t[8])


def ladder(K, a):
    return [1.0 if k == K else 0.0 if k == 0 else math.pow(k / K, 1.0 / a) for k in range(K, -1, -1)]


def estimates(betas, series):
    """lnZ_ss, lnZ_ti and the per-rung terms from the rungs' series, in the order visited (beta from 1 down to 0)"""
    K = len(betas) - 1
    terms, ss, ti = [0.0], 0.0, 0.0
    for i in range(1, K + 1):                   # rung k = K - i: its own samples, the step up to the rung above
        d = betas[i - 1] - betas[i]
        x = d * np.asarray(series[i])
        m = x.max()
        terms.append(m + math.log(np.exp(x - m).mean()))
        ss += terms[-1]
        ti += d * (np.mean(series[i]) + np.mean(series[i - 1])) / 2
    return ss, ti, terms


# ---------------------------------------------------------------- F
def test_f_formulas_reproduce_the_engine(hostemu, tmp_path):
    import gphocs_amd as G
    _, lib = hostemu
    ctl = U.write_toy(str(tmp_path))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        pk = G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)
    assert (pk.n, pk.K, pk.Kc, pk.B, pk.L) == (2, 3, 2, 0, len(U.TOY_DIFFS))
    assert (pk.thetaAlpha[2], pk.thetaBeta[2]) == U.TOY_THETA and (pk.ageAlpha[2], pk.ageBeta[2]) == U.TOY_TAU
    s = G.Sampler(pk, lib=lib)
    s.initialize()
    s.enable_gene_trees(1)
    for it in range(50):
        s.iteration(it)
    s.sample_gene_trees(49)
    t, st = s.gene_trees(), s.state()
    s.close()
    T, tau, theta = t["age"][0][:, 2], st["popAge"][2], st["theta"][2]
    assert np.all(t["root"][0] == 2) and np.all(T > tau) and len(set(T.tolist())) == len(U.TOY_DIFFS)
    assert np.max(np.abs(t["dataLnL"][0] - U.toy_data_lnl(T))) <= 1e-10
    assert np.max(np.abs(t["genLnL"][0] - U.toy_gen_lnl(T, tau, theta))) <= 1e-10
    assert abs(st["dataLogLikelihood"] - U.toy_data_lnl(T).sum()) <= 1e-10


@pytest.fixture(scope="module")
def quadrature():
    fine, coarse = U.toy_lnZ(1e-4, 2e-4), U.toy_lnZ(2e-4, 4e-4)
    return fine, abs(fine - coarse)


def check_estimates(lib, d, quadrature, s, sd_ss, sd_ti):
    import gphocs_amd as G
    lnZ, err = quadrature
    U.write_toy(str(d))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        assert G.run_control_file(lib, "toy.ctl", marginal="ml", marginal_steps=ML["K"], marginal_burnin=ML["b"], marginal_samples=s) == 0
    finally:
        os.chdir(cwd)
    rows, ss, ti, K, a = read_table(os.path.join(d, "ml.marginal.tsv"))
    print(f"lnZ_ss {ss!r} lnZ_ti {ti!r} quadrature {lnZ!r} +- {err:.2g}")
    assert K == ML["K"] and a == 0.3 and len(rows) == K + 1
    assert err < 1e-3
    assert abs(ss - lnZ) <= 4 * sd_ss + err
    assert abs(ti - lnZ) <= 4 * sd_ti + err


def test_f_estimates_against_quadrature(hostemu, quadrature, tmp_path):
    check_estimates(hostemu[1], tmp_path, quadrature, ML["s"], SD_SS, SD_TI)


def test_f_no_information_gives_zero(hostemu, tmp_path):
    """a sequence file without information cannot be loaded (a locus needs a pattern), so the pack of identity C is stepped
    down a ladder by hand: every recorded value is exactly 0, and so are both estimates"""
    import gphocs_amd as G
    U.write_toy(str(tmp_path))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        pk = U.scaled_counts(G.Pack.from_control("toy.ctl", lib=hostemu[1]), 0)
    finally:
        os.chdir(cwd)
    betas, series, it = ladder(4, 0.3), [], 0
    sm = G.Sampler(pk, lib=hostemu[1])
    sm.initialize()
    for beta in betas:
        sm.set_beta(beta)
        series.append([])
        for j in range(50):
            sm.iteration(it)
            it += 1
            series[-1].append(sm.state()["dataLogLikelihood"])
    sm.close()
    assert not np.any(np.asarray(series))
    ss, ti, terms = estimates(betas, series)
    assert ss == 0.0 and ti == 0.0 and not any(terms)


# ---------------------------------------------------------------- G
def test_g_run_unchanged_and_table(hostemu, tmp_path):
    """m3 (migration bands; its own burn-in 0 and 120 iterations) with -l, with and without the ladder"""
    path, lib = hostemu
    import gphocs_amd as G
    K, b, s, a = 5, 7, 20, 0.5
    for d in ("plain", "ml"):
        _copy_case("m3", tmp_path / d)
    program(path, tmp_path / "plain", ["-l", "sum.tsv", "m3.ctl"])
    r = program(path, tmp_path / "ml", ["-l", "sum.tsv", "--marginal-likelihood", "out/../ml", "--ml-steps", str(K), "--ml-burnin", str(b),
                                        "--ml-samples", str(s), "--ml-alpha", str(a), "m3.ctl"], ok=False)
    assert not os.path.exists(tmp_path / "ml" / "ml.marginal.tsv")          # (no directory `out`: the run fails at its very end)
    r = program(path, tmp_path / "ml", ["-l", "sum.tsv", "--marginal-likelihood", "ml", "--ml-steps", str(K), "--ml-burnin", str(b),
                                        "--ml-samples", str(s), "--ml-alpha", str(a), "m3.ctl"])
    for f in ("m3.trace", "sum.tsv"):
        want = (tmp_path / "plain" / f).read_bytes()
        assert len(want) > 500 and (tmp_path / "ml" / f).read_bytes() == want
    rows, ss, ti, K_, a_ = read_table(tmp_path / "ml" / "ml.marginal.tsv")
    betas = ladder(K, a)
    assert (K_, a_) == (K, a) and len(rows) == K + 1
    assert [int(x[0]) for x in rows] == list(range(K, -1, -1)) and all(int(x[2]) == s for x in rows)
    assert [x[1] for x in rows] == [float("%.10g" % v) for v in betas]
    assert all(0.0 <= v <= 1.0 for x in rows for v in x[6:]) and any(0.0 < x[6] < 1.0 for x in rows)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Marginal likelihood: lnZ_ss")]
    assert len(line) == 1 and line[0].split()[3] == "%.10g" % ss and line[0].split()[5] == "%.10g" % ti
    assert sum(ln.startswith("rung ") for ln in r.stdout.splitlines()) == K + 1
    # the same ladder by hand: same seed, same bits
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    sm = G.Sampler(pk, lib=lib)
    sm.initialize()
    for it in range(120):
        sm.iteration(it)
    it, series = max(120, pk.startMig + 1), []
    for beta in betas:
        sm.set_beta(beta)
        for j in range(-b, s):
            sm.iteration(it)
            it += 1
            if j == 0:
                series.append([])
            if j >= 0:
                series[-1].append(sm.state()["dataLogLikelihood"])
    sm.close()
    ss2, ti2, terms = estimates(betas, series)
    for x, sr, term in zip(rows, series, terms):
        assert abs(x[3] - np.mean(sr)) <= 1e-9 * abs(x[3])
        assert abs(x[4] - np.std(sr, ddof=1)) <= 1e-8 * x[4]
        assert abs(x[5] - term) <= 1e-9 * max(1.0, abs(term))
    # ten printed digits, and sums taken in another order than the program's
    assert abs(ss - ss2) <= 1e-9 * abs(ss2) and abs(ti - ti2) <= 1e-9 * abs(ti2)


@pytest.mark.parametrize("args,names", [
    (["--ml-steps", "4"], "--ml-steps"), (["--ml-burnin", "5"], "--ml-burnin"), (["--ml-samples", "9"], "--ml-samples"),
    (["--ml-alpha", "0.4"], "--ml-alpha"),
    (["--beta", "0.5", "--marginal-likelihood", "ml"], "--beta"),
    (["--marginal-likelihood", "ml", "--ml-steps", "0"], "--ml-steps"),
    (["--marginal-likelihood", "ml", "--ml-alpha", "0"], "--ml-alpha"), (["--marginal-likelihood", "ml", "--ml-alpha", "-1"], "--ml-alpha"),
    (["--marginal-likelihood", "ml", "--ml-samples", "0"], "--ml-samples"),
    (["--beta", "65"], "--beta"), (["--beta", "-1"], "--beta")])
def test_g_usage_errors(hostemu, tmp_path, args, names):
    _copy_case("m3", tmp_path)
    r = program(hostemu[0], tmp_path, args + ["m3.ctl"], ok=False)
    assert names in r.stderr and "Starting MCMC" not in r.stdout
    assert not os.path.exists(tmp_path / "m3.trace") and not os.path.exists(tmp_path / "ml.marginal.tsv")


@pytest.mark.parametrize("options,names", [
    (dict(marginal_steps=4), "--ml-steps"), (dict(marginal_burnin=5), "--ml-burnin"), (dict(marginal_samples=9), "--ml-samples"),
    (dict(marginal_alpha=0.4), "--ml-alpha"), (dict(beta=0.5, marginal="ml"), "--beta"), (dict(marginal="ml", marginal_steps=-1), "--ml-steps"),
    (dict(marginal="ml", marginal_alpha=-1.0), "--ml-alpha"), (dict(marginal="ml", marginal_samples=-1), "--ml-samples"), (dict(beta=65.0), "--beta")])
def test_g_library_refuses_the_same(hostemu, tmp_path, capfd, options, names):
    import gphocs_amd as G
    _copy_case("m3", tmp_path)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert G.run_control_file(hostemu[1], "m3.ctl", **options) == -1        # GPH_EARG
    finally:
        os.chdir(cwd)
    assert names in capfd.readouterr().err and not os.path.exists(tmp_path / "m3.trace")


def test_g_failed_run_leaves_no_table(hostemu, tmp_path):
    """a table of an earlier run is gone after a run that fails (here: the trace file cannot be opened)"""
    ctl = open(os.path.join(GOLDEN, "m3.ctl")).read().replace("m3.trace", "nowhere/m3.trace")
    _copy_case("m3", tmp_path, ctl_text=ctl)
    (tmp_path / "ml.marginal.tsv").write_text("stale\n")
    program(hostemu[0], tmp_path, ["--marginal-likelihood", "ml", "--ml-steps", "2", "--ml-burnin", "1", "--ml-samples", "2", "m3.ctl"], ok=False)
    assert not os.path.exists(tmp_path / "ml.marginal.tsv")


# ---------------------------------------------------------------- H
def doubled_seq(src, dst):
    """every locus's alignment concatenated with itself: twice the count of every pattern, in the same pattern order"""
    lines = open(src).read().split("\n")
    out, i = [lines[0]], 1
    while i < len(lines):
        t = lines[i].split()
        if len(t) == 3 and t[1].isdigit() and t[2].isdigit():
            out.append("%s %s %d" % (t[0], t[1], 2 * int(t[2])))
            for ln in lines[i + 1:i + 1 + int(t[1])]:
                name, seq = ln.split()
                assert len(seq) == int(t[2])
                out.append(name + "\t" + seq + seq)
            i += 1 + int(t[1])
        else:
            out.append(lines[i])
            i += 1
    open(dst, "w").write("\n".join(out))


def parameter_columns(trace):
    lines = open(trace).read().splitlines()
    assert len(lines) > 100
    return [lines[0].rsplit("\t", 2)[0]] + [ln.split("\t\t")[0] for ln in lines[1:]]


def test_h_beta_option(hostemu, tmp_path):
    """k3 (12 leaves, 2 migration bands, burn-in 13; here 150 iterations, every one sampled): the one golden whose doubled sequence
    file is the doubled pack.  In the others a locus or two come out with another number of patterns -- the alignment
    processor does not treat a heterozygous column that occurs twice as it treats one that occurs once -- and the pack read
    from the doubled file is checked here for that reason"""
    import gphocs_amd as G
    path, lib = hostemu
    name = "k3"
    ctl = open(os.path.join(GOLDEN, name + ".ctl")).read()
    ctl = re.sub(r"mcmc-iterations\s+24", "mcmc-iterations 150", re.sub(r"mcmc-sample-skip\s+2", "mcmc-sample-skip 0", ctl))
    for d in ("plain", "one", "half"):
        _copy_case(name, tmp_path / d, ctl_text=ctl)
    doubled_seq(os.path.join(GOLDEN, name + ".seq"), tmp_path / "half" / (name + ".seq"))
    packs, cwd = [], os.getcwd()
    for d in ("plain", "half"):
        os.chdir(tmp_path / d)
        try:
            packs.append(G.Pack.from_control(name + ".ctl", lib=lib))
        finally:
            os.chdir(cwd)
    assert np.array_equal(packs[0].pattern_offsets, packs[1].pattern_offsets) and np.array_equal(packs[0].leafcodes, packs[1].leafcodes)
    assert np.array_equal(packs[0].numPhases, packs[1].numPhases) and np.array_equal(2 * packs[0].counts, packs[1].counts)
    r0 = program(path, tmp_path / "plain", [name + ".ctl"])
    r1 = program(path, tmp_path / "one", ["--beta", "1", name + ".ctl"])
    rh = program(path, tmp_path / "half", ["--beta", "0.5", name + ".ctl"])
    want = (tmp_path / "plain" / (name + ".trace")).read_bytes()
    assert (tmp_path / "one" / (name + ".trace")).read_bytes() == want
    assert parameter_columns(tmp_path / "half" / (name + ".trace")) == parameter_columns(tmp_path / "plain" / (name + ".trace"))
    assert (tmp_path / "half" / (name + ".trace")).read_bytes() != want            # the likelihood columns are the doubled file's own
    assert "Power posterior" not in r0.stdout and r1.stdout.count("Power posterior: beta = 1 ") == 1
    assert rh.stdout.count("Power posterior: beta = 0.5 ") == 1


def test_h_beta_zero_is_the_prior(hostemu, tmp_path):
    """--beta 0 on the toy model prints the parameters of the chain on the pack without information (identity C)"""
    import gphocs_amd as G
    path, lib = hostemu
    U.write_toy(str(tmp_path), burnin=0)
    r = program(path, tmp_path, ["--beta", "0", "toy.ctl"])
    assert r.stdout.count("(the prior)") == 1
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        pk = U.scaled_counts(G.Pack.from_control("toy.ctl", lib=lib), 0)
    finally:
        os.chdir(cwd)
    sm = G.Sampler(pk, lib=lib)
    sm.initialize()
    want, pv = [], np.zeros(pk.numParameters)
    for it in range(400):
        sm.iteration(it)
        assert sm.lib.gph_mcmc_param_vals(sm.mcmc, pv.ctypes.data, pk.numParameters) == 0
        want.append("%d\t" % it + "\t".join("%8.5f" % (v * f) for v, f in zip(pv, pk.printFactors)))
    sm.close()
    assert parameter_columns(tmp_path / "toy.trace")[1:] == want


def test_g_two_ranks_write_one_table(hostemu, tmp_path):
    """the ladder over two ranks (shared-memory communicator): every rank steps it with the same beta, rank 0 alone writes,
    there are no parts, and the table is the one-rank table up to the order of the sums over loci"""
    import gphocs_amd as G
    from sampler_util import run_ranks
    path, lib = hostemu
    options = dict(marginal="ml", marginal_steps=3, marginal_burnin=4, marginal_samples=12, marginal_alpha=0.5)
    run_ranks(path, "m3", 2, tmp_path / "two", **options)
    _copy_case("m3", tmp_path / "one")
    cwd = os.getcwd()
    os.chdir(tmp_path / "one")
    try:
        assert G.run_control_file(lib, "m3.ctl", **options) == 0
    finally:
        os.chdir(cwd)
    assert sorted(f for f in os.listdir(tmp_path / "two") if f.startswith("ml")) == ["ml.marginal.tsv"]
    one, two = read_table(tmp_path / "one" / "ml.marginal.tsv"), read_table(tmp_path / "two" / "ml.marginal.tsv")
    assert len(two[0]) == 4 and [r[1] for r in two[0]] == [float("%.10g" % v) for v in ladder(3, 0.5)]
    for a, b in zip(one[0], two[0]):
        assert a[:3] == b[:3] and a[6:] == b[6:]                                  # the same decisions
        assert all(abs(x - y) <= 1e-9 * max(1.0, abs(x)) for x, y in zip(a[3:6], b[3:6]))
    assert abs(one[1] - two[1]) <= 1e-9 * abs(one[1]) and abs(one[2] - two[2]) <= 1e-9 * abs(one[2])
