// gph_exchange.h -- two engines exchange their chain STATES (Metropolis-coupled chains: gph_mc3.h runs the group).
//
// Included by gph_engine.hip inside its extern "C" block, behind everything it calls.  One text for both builds; the one thing
// that differs, the ordering of the two engines' streams, is exchange_order() of gph_backend.h.
//
// What a chain's state is, and where it lives:
//   per locus   dev.pages     genealogy, event chains, statistics, generator triple, likelihoods, locus rate of every locus
//               dev.cond      the conditional arrays (both halves of the double buffer; the page says which half is current)
//               dev.stats     the compact copy of the pages' statistics: gph_engine_get_totals reduces it WITHOUT a kernel that
//                             rewrites it first, so it travels with the pages it mirrors
//               dev.ra_kprev  draws each locus consumed in its last sweep.  A sizing hint only (the draws ahead of a sweep are the
//                             same numbers however many are made), but it describes the loci, not the engine: it travels too
//   above them  the model's parameters, the general generator slot, both likelihood accumulators, the statistics totals, the
//               conflict count and the migration rates as the trace shows them (GphGlobal, host mirror; pushed at the next call)
// What is NOT exchanged, because every launch that reads it has a launch before it in the same call that writes it:
//   dev.shadow (the evaluated state of a global proposal: written by the evaluate kernel, read by the finish that follows -- and
//   the finishes that are owed run before the exchange, below), dev.out (a launch's per-locus outputs, reduced right behind
//   it), dev.ra_draws / ra_ckpt / ra_tail (rewritten by the pass in front of the next sweep once ra_b_valid is down), the
//   locus-rate records and scratch (d_lrec .. d_ref_page: refilled by every update from the pages), d_mutRate (read by k_init
//   only; a running chain's rates are in its pages), d_part / d_red (reduction scratch).
// What stays with the engine by definition: beta, the step sizes, the priors, the accept counters, the log period, every
// sampler's buffers, the timing and class counters, cfg, the streams.
//
// Owed work.  The commit / revert of a decided tau or sample-age proposal (fin_owed) and the commit of an accepted mixing
// proposal (mix_owed) read the shadow pages and the pending proposal in the chain state: they RUN before the exchange, as
// kernels of their own on the engine that took the decision (sample_settle, as in front of a sample).  A deferred
// synchronizeEvents pass (sync_pending) reads nothing but the pages it corrects: the flag is CARRIED ACROSS with them and the
// pass rides at the head of the next sweep of whichever engine holds the pages then, as it would have without an exchange.
//
// Order.  exchange_order() makes each engine's stream wait, through events, for what the other's streams still hold for the
// pages they give away (a finish queued just now; a pass of k_rng_ahead behind the last sweep, which reads the pages on a
// stream of its own).  The draws of such a pass belong to pages the engine no longer holds: ra_b_valid goes down on both sides.

// the two engines can hold each other's state: same device and library, same loci in the same slots
static bool exchange_compatible(const gph_engine *a, const gph_engine *b)
{
  if (a->cfg.device != b->cfg.device || a->cfg.L_total != b->cfg.L_total || a->cfg.locus_begin != b->cfg.locus_begin) return false;
  if (a->cfg.n != b->cfg.n || a->cfg.K != b->cfg.K || a->cfg.Kc != b->cfg.Kc || a->cfg.B != b->cfg.B || a->cfg.rootPop != b->cfg.rootPop) return false;
  if (a->popFather != b->popFather || a->samplesPerPop != b->samplesPerPop || a->bandSrc != b->bandSrc || a->bandTgt != b->bandTgt) return false;
  if (a->L != b->L || memcmp(&a->lay, &b->lay, sizeof a->lay) != 0) return false;
  if (a->pages_bytes != b->pages_bytes || a->cond_bytes != b->cond_bytes || a->var_rates != b->var_rates) return false;
  if (a->h_orig != b->h_orig || a->h_P != b->h_P || a->h_cond_off != b->h_cond_off || a->buckets.size() != b->buckets.size()) return false;
  if (a->dev.ra_M != b->dev.ra_M || a->dev.ra_cshift != b->dev.ra_cshift) return false;
  return true;
}

// the part of the chain state above the loci, between two host mirrors
static void exchange_global(GphGlobal &A, GphGlobal &B)
{
  std::swap(A.model, B.model);
  std::swap(A.gx, B.gx); std::swap(A.gy, B.gy); std::swap(A.gz, B.gz);
  std::swap(A.logLikelihood, B.logLikelihood);
  std::swap(A.dataLogLikelihood, B.dataLogLikelihood);
  for (int p = 0; p < GPH_MAXK; p++) { std::swap(A.tot_coal[p], B.tot_coal[p]); std::swap(A.tot_ncoal[p], B.tot_ncoal[p]); }
  for (int b = 0; b < GPH_MAXB; b++) {
    std::swap(A.tot_mig[b], B.tot_mig[b]); std::swap(A.tot_nmig[b], B.tot_nmig[b]);
    std::swap(A.migRateShown[b], B.migRateShown[b]);
  }
  std::swap(A.shownValid, B.shownValid);
  std::swap(A.rubberband_conflicts, B.rubberband_conflicts);
}

static int exchange_settle(gph_engine *e)
{
  SETDEV(e);
  int rc;
  if ((rc = flush_pending(e))) return rc;
  if (!e->mirror_current && (rc = finish_sync(e))) return rc;
  return sample_settle(e, SETTLE_CHAIN);
}

int gph_engine_exchange_state(gph_engine *a, gph_engine *b)
{
  if (!a || !b || a == b || !a->initialized || !b->initialized) return GPH_EARG;
  if (a->G_h->error || b->G_h->error) return GPH_EARG;
  if (a->comm || b->comm || a->allreduce || b->allreduce) return GPH_EARG;
  if (!exchange_compatible(a, b)) return GPH_EARG;
  int rc;
  if ((rc = exchange_settle(a)) || (rc = exchange_settle(b))) return rc;
  SETDEV(a);
  if ((rc = exchange_order(a, b))) return rc;
  a->ra_b_valid = b->ra_b_valid = false;
  std::swap(a->dev.pages, b->dev.pages);
  std::swap(a->dev.cond, b->dev.cond);
  std::swap(a->dev.stats, b->dev.stats);
  if (a->dev.ra_kprev && b->dev.ra_kprev) std::swap(a->dev.ra_kprev, b->dev.ra_kprev);
  std::swap(a->sync_pending, b->sync_pending);
  exchange_global(*a->G_h, *b->G_h);
  a->G_dirty = b->G_dirty = true;
  return 0;
}
