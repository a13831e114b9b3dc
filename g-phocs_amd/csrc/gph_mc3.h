// gph_mc3.h -- Metropolis-coupled chains on one device (include/gphocs_hip.h: gph_mcmc_exchange_state, gph_mc3_*).
//
// Included by gph_mcmc.cpp inside its extern "C" block.  C chains, chain c on the power posterior with beta_c for good; at a
// swap point two neighbours exchange their STATES (gph_exchange.h), so chain 0 stays the cold chain and everything that is
// tied to its engine -- trace, samplers, output files -- goes on describing the posterior.  The acceptance ratio
//   r = [p(D|G_j+1)^b_j p(D|G_j)^b_j+1] / [p(D|G_j)^b_j p(D|G_j+1)^b_j+1],  ln r = (b_j - b_j+1) (l_j+1 - l_j)
// leaves prod_c p(D|G_c)^b_c p(G_c|Theta_c) p(Theta_c) invariant (the genealogy likelihoods and the priors cancel).
// Between two swap points the chains are independent: the device build runs one host thread a chain, so their launches sit
// on their own streams at the same time; the host-emulation build, whose model tables are process-wide (gph_backend.h:
// launch_pre), runs them one after the other.  Same bits either way.
extern "C" int gph_engine_exchange_state(gph_engine *a, gph_engine *b);

int gph_mcmc_exchange_state(gph_mcmc *a, gph_mcmc *b)
{
  if (!a || !b || a == b) return GPH_EARG;
  if (a->n != b->n || a->K != b->K || a->Kc != b->Kc || a->B != b->B || a->Ltot != b->Ltot || a->mutRateMode != b->mutRateMode ||
      a->numParameters != b->numParameters) return GPH_EARG;
  int rc = gph_engine_exchange_state(a->e, b->e);
  if (rc) return rc;
  std::swap(a->rateVar, b->rateVar);          /* gph_chain_state.rateVar: the one field of it the driver keeps itself */
  a->paramVals.swap(b->paramVals);            /* what the last iteration recorded of the state */
  return 0;
}

struct gph_mc3 {
  std::vector<gph_mcmc *> chains;
  std::vector<double> betas;
  int32_t swap_every = 1, calls = 0, failed = 0;
  uint32_t x = 11, y = 23, z = 137;           // the group's own generator: the general slot's (utils.c:421-426, 459-470)
  std::vector<int64_t> attempts, accepted;    // pair (c, c + 1)
  std::vector<gph_mc3_swap> log;
};

static double mc3_rndu(gph_mc3 *g)
{
  g->x = 171u * (g->x % 177u) - 2u * (g->x / 177u);
  g->y = 172u * (g->y % 176u) - 35u * (g->y / 176u);
  g->z = 170u * (g->z % 178u) - 63u * (g->z / 178u);
  double r = g->x / 30269.0 + g->y / 30307.0 + g->z / 30323.0;
  return r - (int)r;
}

int gph_mc3_create(gph_mcmc *const *chains, int32_t C, const double *betas, int32_t swap_every, uint32_t swap_seed, gph_mc3 **out)
{
  if (!chains || !betas || !out || C < 2 || C > 16) return GPH_EARG;
  for (int c = 0; c < C; c++) {
    if (!chains[c]) return GPH_EARG;
    for (int d = 0; d < c; d++) if (chains[d] == chains[c]) return GPH_EARG;
  }
  for (int c = 0; c < C; c++) { int rc = gph_mcmc_set_beta(chains[c], betas[c]); if (rc) return rc; }
  gph_mc3 *g = new gph_mc3();
  g->chains.assign(chains, chains + C);
  g->betas.assign(betas, betas + C);
  g->swap_every = swap_every;
  g->z = 170u * (swap_seed % 178u) + 137u;
  g->attempts.assign(C - 1, 0);
  g->accepted.assign(C - 1, 0);
  *out = g;
  return 0;
}

void gph_mc3_destroy(gph_mc3 *g) { delete g; }

int gph_mc3_iteration(gph_mc3 *g, int32_t iteration)
{
  if (!g) return GPH_EARG;
  if (g->failed) return g->failed;
  const int C = (int)g->chains.size();
  const int32_t t = g->calls++;
  if (g->swap_every > 0 && t > 0 && t % g->swap_every == 0) {
    const double u1 = mc3_rndu(g), u2 = mc3_rndu(g);
    int j = (int)(u1 * (C - 1));
    if (j > C - 2) j = C - 2;
    gph_mc3_swap s;
    memset(&s, 0, sizeof s);
    s.call = t; s.lower = j; s.beta_lower = g->betas[j]; s.beta_upper = g->betas[j + 1]; s.u = u2;
    int rc;
    if ((rc = gph_mcmc_get_state(g->chains[j], nullptr, &s.l_lower, nullptr, nullptr, nullptr)) ||
        (rc = gph_mcmc_get_state(g->chains[j + 1], nullptr, &s.l_upper, nullptr, nullptr, nullptr))) return g->failed = rc;
    s.lnr = (s.beta_lower - s.beta_upper) * (s.l_upper - s.l_lower);
    s.accepted = (s.lnr >= 0 || log(u2) < s.lnr) ? 1 : 0;
    g->attempts[j]++;
    if (s.accepted) {
      if ((rc = gph_mcmc_exchange_state(g->chains[j], g->chains[j + 1]))) {
        fprintf(stderr, "gphocs_hip: mc3: chains %d and %d could not exchange their states (status %d)\n", j, j + 1, rc);
        return g->failed = rc;
      }
      g->accepted[j]++;
    }
    g->log.push_back(s);
  }
  std::vector<int> rcs(C, 0);
#ifdef GPH_HOSTEMU
  for (int c = 0; c < C; c++) if ((rcs[c] = gph_mcmc_iteration(g->chains[c], iteration))) break;
#else
  {
    std::vector<std::thread> th;
    th.reserve(C);
    for (int c = 0; c < C; c++) th.emplace_back([g, c, iteration, &rcs]() { rcs[c] = gph_mcmc_iteration(g->chains[c], iteration); });
    for (auto &x : th) x.join();
  }
#endif
  for (int c = 0; c < C; c++)
    if (rcs[c]) {
      fprintf(stderr, "gphocs_hip: mc3: chain %d failed in iteration %d (status %d)\n", c, iteration, rcs[c]);
      return g->failed = rcs[c];
    }
  return 0;
}

int gph_mc3_swap_counts(gph_mc3 *g, int64_t *attempts, int64_t *accepted)
{
  if (!g) return GPH_EARG;
  for (size_t c = 0; c < g->attempts.size(); c++) { if (attempts) attempts[c] = g->attempts[c]; if (accepted) accepted[c] = g->accepted[c]; }
  return 0;
}

int gph_mc3_swap_log(gph_mc3 *g, gph_mc3_swap *out, int64_t max, int64_t *count)
{
  if (!g || !count || max < 0 || (!out && max > 0)) return GPH_EARG;
  *count = (int64_t)g->log.size();
  if (!out) return 0;
  if (max < *count) return GPH_EARG;
  for (size_t i = 0; i < g->log.size(); i++) out[i] = g->log[i];
  return 0;
}
