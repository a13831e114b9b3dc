"""What the power-posterior tests share (test_power_posterior.py on the host build, test_power_posterior_gpu.py on the MI355X).

The oracle cannot heat a chain and does not have to.  The root sum of a locus is sum_p log(avg_p) * count_p in pattern order,
so multiplying every pattern count of a pack by 2 multiplies every locus's data log-likelihood, and every sum of such values
over loci, by exactly 2 in fp64; nothing else in the engine reads the counts.  A chain at beta = 1/2 on the doubled pack
therefore takes, bit for bit, the decisions of the chain at beta = 1 on the pack itself (A), beta = 2 on the pack those of
beta = 1 on the doubled pack (B), and beta = 0 those of a pack whose counts are all 0 (C).  Nothing here has a tolerance."""
import copy
import ctypes as C
import os

import numpy as np

from conftest import GOLDEN

# golden: iterations (the golden's own count) and the proposal kinds with a data term the fixture is there to cover
FIXTURES = {
    "m3": (120, ("coal", "spr", "tau", "mixing")),            # 2 migration bands, high migration: SPR traffic
    "v8": (60, ("coal", "spr", "tau", "mixing", "lrate")),    # locus-mut-rate VAR
    "a7": (100, ("coal", "spr", "tau", "mixing", "sage")),    # one estimated sample age
}
TREE_INT = ("father", "left", "right", "npop", "root", "num_migs", "mig_branch", "mig_band", "mig_spop", "mig_tpop")
TREE_F64 = ("age", "genLnL", "mig_age")


FT_MIXING = 0.1     # the goldens' own finetune-mixing, 0.003, is never rejected within their iteration counts


def load(name):
    """the golden's pack, with a mixing step wide enough for the chain to reject some"""
    import gphocs_amd as G
    p = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    p.ftMixing = FT_MIXING
    return p


def scaled_counts(pack, factor):
    """a copy of the pack with every pattern count multiplied by factor (2: doubled; 0: a pack with no information)"""
    q = copy.copy(pack)
    q.counts = np.ascontiguousarray(pack.counts * factor, dtype=pack.counts.dtype)
    assert int(q.counts.max(initial=0)) < 65535          # the 16-bit count form stays available
    return q


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def run(lib, pack, iters, beta=None, beta_from=0, dump=None):
    """one chain of `iters` iterations from the pack's seed; beta (None: set_beta is never called) is set before initialize
    when beta_from == 0, else in front of iteration beta_from.  Everything the comparisons need, fp64 values as bit patterns."""
    import gphocs_amd as G
    s = G.Sampler(pack, lib=lib)
    try:
        if beta is not None and beta_from == 0:
            s.set_beta(beta)
            assert s.beta == beta
        s.initialize()
        s.enable_gene_trees(1)
        for it in range(iters):
            if beta is not None and beta_from == it and it > 0:
                s.set_beta(beta)
            s.iteration(it)
        s.sample_gene_trees(iters - 1)
        t = s.gene_trees()
        npar = pack.numParameters + 1
        pv = np.zeros(npar)
        assert s.lib.gph_mcmc_param_vals(s.mcmc, pv.ctypes.data, npar) == 0
        tau = (C.c_int64 * 64)()
        assert s.lib.gph_mcmc_tau_accept_counts(s.mcmc, tau) == 0
        lra, rv = C.c_int64(), C.c_double()
        assert s.lib.gph_mcmc_locus_rate_state(s.mcmc, C.byref(lra), C.byref(rv)) == 0
        st = s.state()
        if dump:
            s.dump_state(dump, True)
        r = dict(accept=s.accept_counts(), tau=list(tau)[:pack.K], lrate=lra.value, params=bits(pv), rateVar=bits([rv.value]),
                 theta=bits(st["theta"]), popAge=bits(st["popAge"]), migRate=bits(st["migRate"]),
                 dataLogLikelihood=st["dataLogLikelihood"], treeDataLnL=t["dataLnL"][0].copy(), beta=s.beta)
        for k in TREE_INT:
            r["tree_" + k] = t[k][0].tolist()
        for k in TREE_F64:
            r["tree_" + k] = bits(t[k][0])
        return r
    finally:
        s.close()


def same_chain(a, b):
    """the two runs took the same decisions and hold the same genealogies and parameters, bit for bit (the recorded data
    log-likelihoods are compared by the caller: they differ by the factor of the counts)"""
    for k in ("accept", "tau", "lrate", "params", "rateVar", "theta", "popAge", "migRate"):
        assert a[k] == b[k], k
    for k in TREE_INT + TREE_F64:
        assert a["tree_" + k] == b["tree_" + k], k


def data_scaled(a, b, factor):
    """every recorded data log-likelihood of run b is exactly factor times run a's"""
    assert b["dataLogLikelihood"] == factor * a["dataLogLikelihood"]
    assert np.array_equal(b["treeDataLnL"], factor * a["treeDataLnL"])
    assert factor == 0 or a["dataLogLikelihood"] != 0.0


def covered(pack, iters, r, kinds):
    """at least one accepted and one rejected proposal of every kind the fixture is there to cover, from the accept counters
    of the run (proposals per iteration: n - 1 internal nodes and 2n - 2 branches per locus, one tau per ancestral
    population, one sample age per estimated one, one mixing move, one rate per locus but the first)"""
    L, n, K, Kc = pack.L, pack.n, pack.K, pack.Kc
    acc = r["accept"]
    usa = np.asarray(getattr(pack, "updateSampleAge", np.zeros(K, np.int32)))
    total = dict(coal=iters * L * (n - 1), spr=iters * L * (2 * n - 2), mixing=iters, lrate=iters * (L - 1))
    got = dict(coal=acc[0], spr=acc[2], mixing=acc[6], lrate=r["lrate"])
    for k in kinds:
        if k == "tau":
            assert any(0 < r["tau"][p] < iters for p in range(Kc, K)), ("tau", r["tau"])
        elif k == "sage":
            assert any(usa[p] and 0 < r["tau"][p] < iters for p in range(Kc)), ("sage", r["tau"])
        else:
            assert 0 < got[k] < total[k], (k, got[k], total[k])


# ---------------------------------------------------------------- the model whose marginal likelihood is a small integral
# Two current populations A and B with one haploid sample each, no migration band, TOY_LOCI loci of TOY_SITES sites on which
# the two sequences differ at TOY_DIFFS[l] sites.  A locus's genealogy is one number, the age T_l > tau of the only coalescence,
# in the root population; theta_A and theta_B touch nothing (a lone lineage has no event), so their priors integrate to 1 and
#   Z = int int p(theta) p(tau) prod_l [ int_tau^inf (2/theta) exp(-2 (T - tau) / theta) p(D_l | T) dT ] dtheta dtau
# with theta = theta_root ~ Gamma(TOY_THETA), tau = tau_root ~ Gamma(TOY_TAU) (shape, rate), the pairwise coalescent density
# of the engine's genealogy likelihood (rate 2 / theta per pair) and JC69 for two sequences 2 T apart:
#   p(D_l | T) = (1/4)^n (1/4 + 3/4 e)^(n - d) (1/4 - 1/4 e)^d,  e = exp(-8 T / 3).
TOY_DIFFS = (0, 2, 3, 5, 8, 12)
TOY_SITES = 200
TOY_THETA = (4.0, 400.0)
TOY_TAU = (2.0, 400.0)
TOY_CTL = """GENERAL-INFO-START
	seq-file            toy.seq
	trace-file          toy.trace
	locus-mut-rate          CONST
	num-loci            %(loci)d
	random-seed         %(seed)d
	burn-in             %(burnin)d
	mcmc-iterations	  %(iterations)d
	iterations-per-log  100
	logs-per-line       10
	find-finetunes		FALSE
	finetune-coal-time	0.01
	finetune-mig-time	0.3
	finetune-theta		0.01
	finetune-mig-rate	0.02
	finetune-tau		0.005
	finetune-mixing		0.3
	tau-theta-print		1.0
	tau-theta-alpha		%(ta)r
	tau-theta-beta		%(tb)r
	mig-rate-print		1.0
	mig-rate-alpha		0.002
	mig-rate-beta		0.00001
GENERAL-INFO-END
CURRENT-POPS-START
	POP-START
		name		A
		samples		a h
	POP-END
	POP-START
		name		B
		samples		b h
	POP-END
CURRENT-POPS-END
ANCESTRAL-POPS-START
	POP-START
		name			root
		children		A		B
		tau-initial	0.005
		tau-alpha		%(aa)r
		tau-beta		%(ab)r
		finetune-tau			0.005
	POP-END
ANCESTRAL-POPS-END
"""


def write_toy(d, seed=12345, burnin=200, iterations=400):
    """toy.ctl and toy.seq in directory d"""
    base = "ACGT" * (TOY_SITES // 4)
    sub = {"A": "C", "C": "G", "G": "T", "T": "A"}
    with open(os.path.join(d, "toy.seq"), "w") as f:
        f.write("%d\n\n" % len(TOY_DIFFS))
        for i, k in enumerate(TOY_DIFFS):
            a, b = base, "".join(sub[c] if j < k else c for j, c in enumerate(base))
            f.write("locus%d 2 %d\na\t%s\nb\t%s\n\n" % (i + 1, len(a), a, b))
    with open(os.path.join(d, "toy.ctl"), "w") as f:
        f.write(TOY_CTL % dict(loci=len(TOY_DIFFS), seed=seed, burnin=burnin, iterations=iterations, ta=TOY_THETA[0], tb=TOY_THETA[1],
                               aa=TOY_TAU[0], ab=TOY_TAU[1]))
    return os.path.join(d, "toy.ctl")


def toy_data_lnl(T, diffs=TOY_DIFFS, sites=TOY_SITES):
    """ln p(D_l | T_l) per locus"""
    T, d = np.asarray(T, dtype=np.float64), np.asarray(diffs, dtype=np.float64)
    e = np.exp(-8.0 * T / 3.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return sites * np.log(0.25) + (sites - d) * np.log(0.25 + 0.75 * e) + np.where(d > 0, d * np.log(0.25 - 0.25 * e), 0.0)


def toy_gen_lnl(T, tau, theta):
    """ln p(G_l | Theta) per locus: one coalescence of two lineages at age T in the root population"""
    return np.log(2.0 / theta) - 2.0 * (np.asarray(T) - tau) / theta


def _gamma_lnpdf(x, shape, rate):
    import math
    with np.errstate(divide="ignore"):
        return shape * math.log(rate) - math.lgamma(shape) + (shape - 1.0) * np.log(x) - rate * x


def toy_lnZ(h_T=1e-4, h_theta=2e-4, T_max=0.4, theta_max=0.08):
    """ln Z of the model above by the trapezoid rule in all three dimensions, in logarithms: T and tau on the grid j h_T up to
    T_max (beyond it p(D | T) exp(-2 T / theta) is below 1e-30 of its peak for every locus), theta on i h_theta up to theta_max
    (its prior density is below 1e-14 of its peak there)"""
    T = np.arange(0, int(round(T_max / h_T)) + 1) * h_T
    lik = np.stack([toy_data_lnl(T, diffs=(d,))[...] for d in TOY_DIFFS])          # [L, NT]
    ln_p_tau = _gamma_lnpdf(T, *TOY_TAU)
    wT = np.full(T.size, h_T)
    wT[0] = wT[-1] = h_T / 2
    thetas = np.arange(1, int(round(theta_max / h_theta)) + 1) * h_theta
    F = np.empty(thetas.size)
    for i, th in enumerate(thetas):
        A = lik - 2.0 * T / th
        seg = np.log(h_T / 2) + np.logaddexp(A[:, :-1], A[:, 1:])                  # [L, NT - 1]
        C = np.full(A.shape, -np.inf)
        C[:, :-1] = np.logaddexp.accumulate(seg[:, ::-1], axis=1)[:, ::-1]         # ln int_{T_j}^{T_max}
        ln_I = np.log(2.0 / th) + 2.0 * T / th + C                                 # [L, NT]: by tau = T_j
        with np.errstate(divide="ignore"):
            F[i] = np.logaddexp.reduce(np.log(wT) + ln_p_tau + ln_I.sum(axis=0))
    w = np.full(thetas.size, h_theta)
    w[-1] = h_theta / 2                                                            # (the integrand is 0 at theta = 0)
    return float(np.logaddexp.reduce(np.log(w) + _gamma_lnpdf(thetas, *TOY_THETA) + F))
