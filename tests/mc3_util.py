"""What the tests of the Metropolis-coupled chains share (test_mc3.py on the host build, test_mc3_gpu.py on the MI355X).

The emulation.  Two chains that differ in beta only and exchange their STATES are the same two chains exchanging their BETAS.
So an MC3 run is rebuilt here from calls that were there before it: C plain Samplers with seeds seed + c, a list that says who
holds which beta, the swap points decided in Python -- the group's generator is the one of rng_ahead_util (numpy), the
logarithm is math.log, the rule is the one of include/gphocs_hip.h -- and every accepted swap carried out as two set_beta
calls.  "The holder of beta_c" here is "chain c" of the MC3 run: same state, bit for bit, after every call.  Nothing here has a
tolerance."""
import copy
import ctypes as C
import math
import os

import numpy as np

import power_posterior_util as U
import rng_ahead_util as R

GPH_EARG = -1
EXCHANGE_PACKS = ("m3", "v8", "a7", "bigp", "x8")     # bands + SPR; VAR (the R lines travel); a sample age; P > 64; 32 leaves, variant x
GROUP_RUNS = {"m3": 120, "v8": 60, "a7": 100}
BETAS = (1.0, 0.7, 0.4)


def load(name):
    import gphocs_amd as G
    if name in U.FIXTURES:
        return U.load(name)
    p = G.Pack.load(os.path.join(U.GOLDEN, name + ".gpk"))
    p.ftMixing = U.FT_MIXING
    return p


def seeded(pack, seed):
    q = copy.copy(pack)
    q.seed = seed
    return q


def sampler(lib, pack, seed, beta=None):
    import gphocs_amd as G
    s = G.Sampler(seeded(pack, seed), lib=lib)
    if beta is not None:
        s.set_beta(beta)
    s.initialize()
    return s


def chain_state(s):
    ch = R.Chain()
    assert s.lib.gph_mcmc_get_chain(s.mcmc, C.byref(ch)) == 0
    return bytes(ch)


def settings(s):
    """what stays with a chain's engine: beta, the accept counters, the tau counters, the locus-rate count"""
    tau = (C.c_int64 * 64)()
    assert s.lib.gph_mcmc_tau_accept_counts(s.mcmc, tau) == 0
    lra = C.c_int64()
    assert s.lib.gph_mcmc_locus_rate_state(s.mcmc, C.byref(lra), None) == 0
    return dict(beta=s.beta, accept=s.accept_counts()[:8], tau=list(tau)[:s.pack.K], lrate=lra.value)


def state_bits(s):
    st = s.state()
    return (U.bits([st["logLikelihood"], st["dataLogLikelihood"]]), U.bits(st["theta"]), U.bits(st["popAge"]), U.bits(st["migRate"]))


def check_ok(s, it):
    ok = C.c_int32()
    assert s.lib.gph_mcmc_check_all(s.mcmc, it, C.byref(ok)) == 0 and ok.value == 1


def per_locus(dump):
    i = dump.index(b"LOCUS ")
    return dump[i:]


# ---------------------------------------------------------------- the group's generator and rule, a second time
class SwapRng:
    def __init__(self, seed):
        self.s = np.array([[11, 23, 170 * ((seed & 0xffffffff) % 178) + 137]], dtype=np.uint64)

    def u(self):
        self.s = R.step(self.s)
        return float(R.draw_bits(self.s).view(np.float64)[0])


def decide(C_, betas, ell, u1, u2):
    """(lower, lnr, accepted) of a swap point; ell[c] = dataLogLikelihood of the holder of betas[c]"""
    j = min(int(u1 * (C_ - 1)), C_ - 2)
    lnr = (betas[j] - betas[j + 1]) * (ell[j + 1] - ell[j])
    acc = lnr >= 0 or (math.log(u2) if u2 > 0 else -math.inf) < lnr
    return j, lnr, bool(acc)


class Emulation:
    """C plain samplers; holder[c] = the sampler that holds betas[c]"""

    def __init__(self, lib, pack, betas, swap_every, swap_seed=None, prepare=None):
        self.betas = list(betas)
        self.C = len(betas)
        self.s = [sampler(lib, pack, pack.seed + c, b) for c, b in enumerate(betas)]
        self.holder = list(range(self.C))
        self.swap_every = swap_every
        self.rng = SwapRng(pack.seed + self.C if swap_seed is None else swap_seed)
        self.calls = 0
        self.log = []
        self.cold = []            # the holder of betas[0] during every call
        if prepare:
            for x in self.s:
                prepare(x)

    def iteration(self, it):
        t = self.calls
        self.calls += 1
        if self.swap_every > 0 and t > 0 and t % self.swap_every == 0:
            u1, u2 = self.rng.u(), self.rng.u()
            ell = [self.s[self.holder[c]].state()["dataLogLikelihood"] for c in range(self.C)]
            j, lnr, acc = decide(self.C, self.betas, ell, u1, u2)
            self.log.append(dict(call=t, lower=j, beta_lower=self.betas[j], beta_upper=self.betas[j + 1], l_lower=ell[j], l_upper=ell[j + 1],
                                 lnr=lnr, u=u2, accepted=int(acc)))
            if acc:
                self.holder[j], self.holder[j + 1] = self.holder[j + 1], self.holder[j]
                self.s[self.holder[j]].set_beta(self.betas[j])
                self.s[self.holder[j + 1]].set_beta(self.betas[j + 1])
        self.cold.append(self.holder[0])
        for x in self.s:
            x.iteration(it)

    def of(self, c):
        return self.s[self.holder[c]]

    def close(self):
        for x in self.s:
            x.close()


def log_bits(log):
    return [(e["call"], e["lower"], U.bits([e["beta_lower"], e["beta_upper"], e["l_lower"], e["l_upper"], e["lnr"], e["u"]]), e["accepted"])
            for e in log]


def trace_lines(path):
    """iteration -> the TRACE record line of a record file"""
    out = {}
    with open(path) as f:
        for ln in f:
            if ln.startswith("TRACE "):
                out[int(ln.split()[1])] = ln
    return out


# ---------------------------------------------------------------- A: the exchange alone
def check_exchange(lib, name, tmp, seed_shift=0):
    pack = load(name)
    seed = pack.seed + seed_shift
    d = lambda s, tag: R.dump(s, os.path.join(str(tmp), tag), True)      # noqa: E731
    a, b = sampler(lib, pack, seed, 1.0), sampler(lib, pack, seed + 1, 0.5)
    x, y = sampler(lib, pack, seed, 1.0), sampler(lib, pack, seed + 1, 0.5)          # the emulation
    try:
        for it in range(7):
            for s in (a, b, x, y):
                s.iteration(it)
        a0, b0 = d(a, "a0"), d(b, "b0")
        assert a0 != b0 and per_locus(a0) != per_locus(b0) and len(a0) > 1000
        if name == "v8":
            assert b"\nR " in a0
        ca, cb, sa, sb, ka, kb = chain_state(a), chain_state(b), state_bits(a), state_bits(b), settings(a), settings(b)
        assert ca != cb and sa != sb
        a.exchange_state(b)
        a1, b1 = d(a, "a1"), d(b, "b1")
        assert a1 == b0 and b1 == a0                        # every line, the per-locus ones and those above them
        assert chain_state(a) == cb and chain_state(b) == ca and state_bits(a) == sb and state_bits(b) == sa
        assert settings(a) == ka and settings(b) == kb and a.beta == 1.0 and b.beta == 0.5
        check_ok(a, 6), check_ok(b, 6), check_ok(x, 6), check_ok(y, 6)
        x.set_beta(0.5), y.set_beta(1.0)
        for it in range(7, 12):
            for s in (a, b, x, y):
                s.iteration(it)
        assert d(a, "a2") == d(y, "y2") and d(b, "b2") == d(x, "x2")
        assert d(a, "a2") != d(b, "b2")
    finally:
        for s in (a, b, x, y):
            s.close()


def check_exchange_twice(lib, name, tmp):
    """exchanged twice in a row, a pair equals one that never was"""
    pack = load(name)
    d = lambda s, tag: R.dump(s, os.path.join(str(tmp), tag), True)      # noqa: E731
    a, b = sampler(lib, pack, pack.seed, 1.0), sampler(lib, pack, pack.seed + 1, 0.5)
    x, y = sampler(lib, pack, pack.seed, 1.0), sampler(lib, pack, pack.seed + 1, 0.5)
    try:
        for it in range(7):
            for s in (a, b, x, y):
                s.iteration(it)
        a.exchange_state(b)
        b.exchange_state(a)
        assert d(a, "a") == d(x, "x") and d(b, "b") == d(y, "y")
        for it in range(7, 10):
            for s in (a, b, x, y):
                s.iteration(it)
        assert d(a, "a") == d(x, "x") and d(b, "b") == d(y, "y")
        assert a.accept_counts() == x.accept_counts() and b.accept_counts() == y.accept_counts()
    finally:
        for s in (a, b, x, y):
            s.close()


def check_exchange_repeated(lib, tmp, first=7, last=20):
    """m3: an exchange in front of every iteration first .. last; some follow an accepted mixing proposal (its commit is still
    owed to the pages), some a rejected one.  Returns what followed what, per engine."""
    pack = load("m3")
    d = lambda s, tag: R.dump(s, os.path.join(str(tmp), tag), True)      # noqa: E731
    a, b = sampler(lib, pack, pack.seed, 1.0), sampler(lib, pack, pack.seed + 1, 0.5)
    x, y = sampler(lib, pack, pack.seed, 1.0), sampler(lib, pack, pack.seed + 1, 0.5)
    after = {"a": [], "b": []}
    try:
        for it in range(last + 3):
            if first <= it <= last:
                a.exchange_state(b)
                bx, by = x.beta, y.beta
                x.set_beta(by), y.set_beta(bx)
            m = [s.accept_counts()[6] for s in (a, b)]
            for s in (a, b, x, y):
                s.iteration(it)
            if first - 1 <= it < last:                       # the mixing proposals the next exchange follows
                after["a"].append(a.accept_counts()[6] - m[0])
                after["b"].append(b.accept_counts()[6] - m[1])
        n = last - first + 1
        pa, pb = (a, b) if n % 2 == 0 else (b, a)
        assert d(pa, "a") == d(x, "x") and d(pb, "b") == d(y, "y")
        check_ok(a, last + 2), check_ok(b, last + 2)
    finally:
        for s in (a, b, x, y):
            s.close()
    for k in ("a", "b"):
        assert 1 in after[k] and 0 in after[k], after          # asserted, so that the owed commit cannot go untested
    return after


def check_refusals(lib, tmp):
    """every refusal that can be produced from here returns GPH_EARG and changes no byte of either dump"""
    import gphocs_amd as G
    pack, other = load("m3"), load("a7")
    d = lambda s, tag: R.dump(s, os.path.join(str(tmp), tag), True)      # noqa: E731
    a, b = sampler(lib, pack, pack.seed, 1.0), sampler(lib, pack, pack.seed + 1, 0.5)
    fresh = G.Sampler(seeded(pack, pack.seed), lib=lib)                     # not initialised
    hooked = G.Sampler(seeded(pack, pack.seed), lib=lib, allreduce=lambda s, m: None)
    hooked.initialize()
    o = sampler(lib, other, other.seed)                                     # another data set: L, layout
    comm = a.lib.gph_comm_create_shm(("/gphocs-mc3x-%d" % os.getpid()).encode(), 0, 1)
    assert comm
    joined = G.Sampler(seeded(pack, pack.seed), lib=lib, comm=comm)         # a communicator, even of one rank
    joined.initialize()
    try:
        for it in range(3):
            a.iteration(it), b.iteration(it), o.iteration(it), hooked.iteration(it)
        a0, b0, o0, h0 = d(a, "a"), d(b, "b"), d(o, "o"), d(hooked, "h")
        lib = a.lib
        ex = lib.gph_mcmc_exchange_state
        assert ex(a.mcmc, a.mcmc) == GPH_EARG
        assert ex(a.mcmc, None) == GPH_EARG and ex(None, a.mcmc) == GPH_EARG
        assert ex(a.mcmc, fresh.mcmc) == GPH_EARG and ex(fresh.mcmc, a.mcmc) == GPH_EARG
        assert ex(a.mcmc, hooked.mcmc) == GPH_EARG and ex(hooked.mcmc, a.mcmc) == GPH_EARG
        assert lib.gph_engine_exchange_state(a.engine, hooked.engine) == GPH_EARG
        assert ex(a.mcmc, joined.mcmc) == GPH_EARG and ex(joined.mcmc, a.mcmc) == GPH_EARG
        assert lib.gph_engine_exchange_state(a.engine, a.engine) == GPH_EARG
        if o.lib is a.lib:
            assert ex(a.mcmc, o.mcmc) == GPH_EARG and ex(o.mcmc, a.mcmc) == GPH_EARG
            assert lib.gph_engine_exchange_state(a.engine, o.engine) == GPH_EARG
        assert (d(a, "a"), d(b, "b"), d(o, "o"), d(hooked, "h")) == (a0, b0, o0, h0)
    finally:
        for s in (a, b, fresh, hooked, o, joined):
            s.close()
        a.lib.gph_comm_destroy(comm)


# ---------------------------------------------------------------- B, C: the group against the emulation
def check_group(lib, name, iters, tmp, betas=BETAS, swap_every=1, trees=False):
    """the MC3 run and its emulation side by side; returns the swap log"""
    import gphocs_amd as G
    pack = load(name)
    C_ = len(betas)
    d = lambda s, tag: R.dump(s, os.path.join(str(tmp), tag), True)      # noqa: E731
    g = G.MC3(pack, betas, swap_every=swap_every, lib=lib)
    emu = Emulation(lib, pack, betas, swap_every, prepare=(lambda s: s.enable_gene_trees(1)) if trees else None)
    try:
        g.chains[0].set_record_file(os.path.join(str(tmp), "mc3.rec"))
        for c, s in enumerate(emu.s):
            s.set_record_file(os.path.join(str(tmp), "emu%d.rec" % c))
        g.initialize()
        assert [s.pack.seed for s in g.chains] == [pack.seed + c for c in range(C_)]
        if trees:
            g.chains[0].enable_gene_trees(1)
        for it in range(iters):
            g.iteration(it)
            emu.iteration(it)
            if trees:
                g.chains[0].sample_gene_trees(it)
                emu.of(0).sample_gene_trees(it)
                t, w = g.chains[0].gene_trees(), emu.of(0).gene_trees()
                for k in U.TREE_INT:
                    assert t[k][0].tolist() == w[k][0].tolist(), (it, k)
                for k in U.TREE_F64 + ("dataLnL",):
                    assert U.bits(t[k][0]) == U.bits(w[k][0]), (it, k)
        for c in range(C_):
            assert g.chains[c].beta == betas[c] == emu.of(c).beta
            assert d(g.chains[c], "g%d" % c) == d(emu.of(c), "e%d" % c), c
        g.chains[0].set_record_file(None)
        for s in emu.s:
            s.set_record_file(None)
        got = trace_lines(os.path.join(str(tmp), "mc3.rec"))
        want = [trace_lines(os.path.join(str(tmp), "emu%d.rec" % c)) for c in range(C_)]
        assert sorted(got) == list(range(iters))
        for it in range(iters):
            assert got[it] == want[emu.cold[it]][it], it
        assert len(set(emu.cold)) > 1                        # the cold state did change hands
        assert np.array_equal(np.sum([s.accept_counts() for s in g.chains], axis=0), np.sum([s.accept_counts() for s in emu.s], axis=0))
        log = g.swap_log()
        assert log_bits(log) == log_bits(emu.log) and len(log) == (iters - 1) // swap_every
        att, acc = g.swap_counts()
        assert att == [sum(1 for e in log if e["lower"] == c) for c in range(C_ - 1)]
        assert acc == [sum(e["accepted"] for e in log if e["lower"] == c) for c in range(C_ - 1)]
        assert 0 < sum(acc) < sum(att), (att, acc)           # at least one accepted and one rejected swap
        return log
    finally:
        g.close()
        emu.close()


# ---------------------------------------------------------------- E: the expected data log-likelihood under the posterior
def toy_lnZ_beta(beta, h_T=1e-4, h_theta=2e-4, T_max=0.4, theta_max=0.08):
    """ln Z(beta) = ln int p(D | G)^beta p(G | Theta) p(Theta) of the toy model: the three-dimensional trapezoid of
    power_posterior_util.toy_lnZ with the factor beta on the data term and nothing else changed"""
    T = np.arange(0, int(round(T_max / h_T)) + 1) * h_T
    lik = beta * np.stack([U.toy_data_lnl(T, diffs=(d,))[...] for d in U.TOY_DIFFS])
    ln_p_tau = U._gamma_lnpdf(T, *U.TOY_TAU)
    wT = np.full(T.size, h_T)
    wT[0] = wT[-1] = h_T / 2
    thetas = np.arange(1, int(round(theta_max / h_theta)) + 1) * h_theta
    F = np.empty(thetas.size)
    for i, th in enumerate(thetas):
        A = lik - 2.0 * T / th
        seg = np.log(h_T / 2) + np.logaddexp(A[:, :-1], A[:, 1:])
        Cm = np.full(A.shape, -np.inf)
        Cm[:, :-1] = np.logaddexp.accumulate(seg[:, ::-1], axis=1)[:, ::-1]
        ln_I = np.log(2.0 / th) + 2.0 * T / th + Cm
        with np.errstate(divide="ignore"):
            F[i] = np.logaddexp.reduce(np.log(wT) + ln_p_tau + ln_I.sum(axis=0))
    w = np.full(thetas.size, h_theta)
    w[-1] = h_theta / 2
    return float(np.logaddexp.reduce(np.log(w) + U._gamma_lnpdf(thetas, *U.TOY_THETA) + F))


def toy_expected_lnl(eps=1e-3):
    """E_1[l] = d ln Z / d beta at beta = 1 by a central difference, and its refinement error from halving the grid"""
    fine = (toy_lnZ_beta(1 + eps, 1e-4, 2e-4) - toy_lnZ_beta(1 - eps, 1e-4, 2e-4)) / (2 * eps)
    coarse = (toy_lnZ_beta(1 + eps, 2e-4, 4e-4) - toy_lnZ_beta(1 - eps, 2e-4, 4e-4)) / (2 * eps)
    return fine, abs(fine - coarse)


# ---------------------------------------------------------------- D: the program
REPORT_HEADER = "chain beta seed swapAttempts swapAccepted accCoal accMig accSpr accTheta accMigRate accTau accMixing meanLnL".split()


def program(lib_path, cwd, args, ok=True):
    """the launcher; lib_path None: the product libraries (the MI355X)"""
    import subprocess
    from sampler_util import EXE
    env = dict(os.environ, GPHOCS_HIP_LIB=lib_path) if lib_path else dict(os.environ)
    r = subprocess.run([EXE] + args, cwd=str(cwd), capture_output=True, text=True, timeout=600, env=env)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def read_report(path):
    lines = open(str(path)).read().splitlines()
    assert lines[0].split("\t") == REPORT_HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    t = lines[-1].split()
    assert t[0] == "#" and t[1::2] == ["heat", "every", "attempted", "accepted"]
    return rows, float(t[2]), int(t[4]), int(t[6]), int(t[8])


def pack_of(lib, d, ctl):
    import gphocs_amd as G
    cwd = os.getcwd()
    os.chdir(str(d))
    try:
        return G.Pack.from_control(ctl, lib=lib)
    finally:
        os.chdir(cwd)


def check_program_outputs_unchanged(lib_path, tmp):
    """D1: with the swaps off, chain 0 is the run without --mc3: the trace and every output file, byte for byte"""
    from sampler_util import _copy_case
    outs = ["-l", "sum.tsv", "-s", "cs", "--gene-trees", "gt", "--clades", "cl"]
    for d in ("plain", "mc3"):
        _copy_case("m3", tmp / d)
    program(lib_path, tmp / "plain", outs + ["m3.ctl"])
    r = program(lib_path, tmp / "mc3", ["--mc3", "3", "--mc3-swap-every", "-1"] + outs + ["m3.ctl"])
    files = sorted(f for f in os.listdir(str(tmp / "plain")) if f not in ("m3.ctl", "m3.seq"))
    assert "m3.trace" in files and "sum.tsv" in files and any(f.startswith("cs.") for f in files)
    assert any(f.startswith("gt.") for f in files) and any(f.startswith("cl.") for f in files)
    assert sorted(f for f in os.listdir(str(tmp / "mc3")) if f not in ("m3.ctl", "m3.seq")) == files
    for f in files:
        want = (tmp / "plain" / f).read_bytes()
        assert len(want) > 100 and (tmp / "mc3" / f).read_bytes() == want, f
    assert r.stdout.count("MC3: 3 chains on the ladder") == 1 and "no swaps" in r.stdout
    assert sum(ln.startswith("MC3: chains ") and ln.endswith(": 0 swaps attempted, 0 accepted.") for ln in r.stdout.splitlines()) == 2


def check_program_against_emulation(lib_path, lib, tmp, heat=0.4):
    """D2: the trace of `--mc3 3 --mc3-heat 0.4` against the emulation's beta = 1 holder, the report against its log"""
    from sampler_util import _copy_case
    _copy_case("m3", tmp / "run")
    r = program(lib_path, tmp / "run", ["--mc3", "3", "--mc3-heat", str(heat), "--mc3-report", "out", "m3.ctl"])
    pack = pack_of(lib, tmp / "run", "m3.ctl")
    betas = [1.0 / (1.0 + heat * c) for c in range(3)]
    emu = Emulation(lib, pack, betas, 1)
    try:
        for c, s in enumerate(emu.s):
            s.set_record_file(os.path.join(str(tmp), "emu%d.rec" % c))
        for it in range(120):
            emu.iteration(it)
        for s in emu.s:
            s.set_record_file(None)
        accept = [emu.of(c).accept_counts() for c in range(3)]
    finally:
        emu.close()
    want = [trace_lines(os.path.join(str(tmp), "emu%d.rec" % c)) for c in range(3)]
    got = open(str(tmp / "run" / "m3.trace")).read().splitlines()[1:]
    assert len(got) == 120 and len(set(emu.cold)) > 1
    for ln in got:
        it = int(ln.split("\t")[0])
        w = want[emu.cold[it]][it][len("TRACE "):].rstrip("\n")
        gt, wt = ln.split("\t"), w.split("\t")
        assert gt[:-2] == wt[:-2], (it, ln, w)                 # the parameter columns, character for character
        for a, b in zip(gt[-2:], wt[-2:]):                     # the two likelihood columns: parity_util.compare_trace_files
            assert abs(float(a) - float(b)) <= 1e-9 * abs(float(b)) + 1.000001e-6, (it, ln, w)
    rows, h, every, att, acc = read_report(tmp / "run" / "out.mc3.tsv")
    assert len(rows) == 3 and (h, every) == (heat, 1)
    assert (att, acc) == (len(emu.log), sum(e["accepted"] for e in emu.log)) and 0 < acc < att == 119
    for c, row in enumerate(rows):
        assert row[:3] == [str(c), "%.10g" % betas[c], str(pack.seed + c)]
        n = [sum(1 for e in emu.log if e["lower"] == c), sum(e["accepted"] for e in emu.log if e["lower"] == c)] if c < 2 else [0, 0]
        assert [int(row[3]), int(row[4])] == n
        assert all(0.0 <= float(v) <= 1.0 for v in row[5:12])
    # the acceptance columns are those of the chains' engines: summed over the chains they are the emulation's, summed
    tot = pack.L * (pack.n - 1)
    assert abs(sum(float(r_[5]) for r_ in rows) - sum(a[0] for a in accept) / (120.0 * tot)) <= 1e-9
    assert r.stdout.count("MC3: 3 chains on the ladder") == 1
    pairs = [ln for ln in r.stdout.splitlines() if ln.startswith("MC3: chains ")]
    assert len(pairs) == 2 and all("%s swaps attempted, %s accepted." % (rows[c][3], rows[c][4]) in pairs[c] for c in range(2))


USAGE_ERRORS = [
    (["--mc3", "1"], "--mc3"), (["--mc3", "17"], "--mc3"), (["--mc3", "0"], "--mc3"),
    (["--mc3-heat", "0.2"], "--mc3-heat"), (["--mc3-swap-every", "2"], "--mc3-swap-every"), (["--mc3-report", "out"], "--mc3-report"),
    (["--mc3", "2", "--mc3-heat", "-1", "--mc3-report", "out"], "--mc3-heat"),
    (["--mc3", "2", "-g", "2", "--mc3-report", "out"], "--mc3"), (["--mc3", "2", "--beta", "0.5", "--mc3-report", "out"], "--mc3"),
    (["--mc3", "2", "--marginal-likelihood", "ml", "--mc3-report", "out"], "--mc3")]
LIBRARY_REFUSALS = [
    (dict(mc3=1), "--mc3"), (dict(mc3=17), "--mc3"), (dict(mc3=-2), "--mc3"), (dict(mc3_heat=0.2), "--mc3-heat"),
    (dict(mc3_swap_every=2), "--mc3-swap-every"), (dict(mc3_report="out"), "--mc3-report"), (dict(mc3=2, mc3_heat=-1.0, mc3_report="out"), "--mc3-heat"),
    (dict(mc3=2, beta=0.5, mc3_report="out"), "--mc3"), (dict(mc3=2, marginal="ml", mc3_report="out"), "--mc3"),
    (dict(mc3=2, comm=True, mc3_report="out"), "--mc3")]


def check_usage_error(lib_path, tmp, args, names):
    from sampler_util import _copy_case
    _copy_case("m3", tmp)
    r = program(lib_path, tmp, args + ["m3.ctl"], ok=False)
    assert names in r.stderr and "Starting MCMC" not in r.stdout and "Reading control settings" not in r.stdout
    assert sorted(os.listdir(str(tmp))) == ["m3.ctl", "m3.seq"]


def check_library_refusal(lib, tmp, capfd, options, names):
    import gphocs_amd as G
    from sampler_util import _copy_case
    _copy_case("m3", tmp)
    options = dict(options)
    comm = None
    if options.get("comm"):
        comm = lib.gph_comm_create_shm(("/gphocs-mc3-%d" % os.getpid()).encode(), 0, 1)
        assert comm
        options["comm"] = comm
    cwd = os.getcwd()
    os.chdir(str(tmp))
    try:
        assert G.run_control_file(lib, "m3.ctl", **options) == GPH_EARG
    finally:
        os.chdir(cwd)
        if comm:
            lib.gph_comm_destroy(comm)
    assert names in capfd.readouterr().err and sorted(os.listdir(str(tmp))) == ["m3.ctl", "m3.seq"]


def check_failed_run_leaves_no_report(lib_path, tmp):
    """a report of an earlier run is gone after a run that fails (here: the trace file cannot be opened)"""
    from sampler_util import _copy_case
    ctl = open(os.path.join(U.GOLDEN, "m3.ctl")).read().replace("m3.trace", "nowhere/m3.trace")
    _copy_case("m3", tmp, ctl_text=ctl)
    (tmp / "out.mc3.tsv").write_text("stale\n")
    program(lib_path, tmp, ["--mc3", "2", "--mc3-report", "out", "m3.ctl"], ok=False)
    assert not os.path.exists(str(tmp / "out.mc3.tsv"))


# ---------------------------------------------------------------- E: the cold chain still samples the posterior
TOY = dict(chains=4, heat=2.0, burnin=500, samples=2000, seed=12345)


def check_cold_chain_samples_posterior(lib, tmp, sd_plain):
    """`--mc3 4` on the toy model: every pair's accepted fraction in [0.1, 0.9] (asserted), and the mean of the data
    log-likelihood over the trace against E_1[l] by quadrature, within 4 standard deviations of the plain chain's mean plus
    the quadrature's refinement error"""
    import gphocs_amd as G
    want, err = toy_expected_lnl()
    U.write_toy(str(tmp), seed=TOY["seed"], burnin=TOY["burnin"], iterations=TOY["samples"])
    cwd = os.getcwd()
    os.chdir(str(tmp))
    try:
        assert G.run_control_file(lib, "toy.ctl", mc3=TOY["chains"], mc3_heat=TOY["heat"], mc3_report="toy") == 0
    finally:
        os.chdir(cwd)
    rows, h, every, att, acc = read_report(tmp / "toy.mc3.tsv")
    frac = [int(r[4]) / int(r[3]) for r in rows[:-1]]
    lines = open(str(tmp / "toy.trace")).read().splitlines()
    assert lines[0].split("\t")[-2:] == ["Data-ld-ln", "Full-ld-ln"] and len(lines) == 1 + TOY["samples"]
    # the data log-likelihood l is the LAST column: the trace prints logLikelihood under "Data-ld-ln" and dataLogLikelihood
    # under "Full-ld-ln", as upstream does (GPhoCS.c:1763-1769)
    mean = float(np.mean([float(ln.split("\t")[-1]) for ln in lines[1:]]))
    print(f"accepted fractions {frac}, mean data log-likelihood {mean!r}, quadrature {want!r} +- {err:.2g}, margin {4 * sd_plain + err!r}")
    assert len(rows) == TOY["chains"] and att == TOY["burnin"] + TOY["samples"] - 1
    assert all(0.1 <= f <= 0.9 for f in frac), frac
    assert err < 1e-3
    assert abs(mean - want) <= 4 * sd_plain + err
    return mean
