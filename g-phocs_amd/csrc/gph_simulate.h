// gph_simulate.h -- k_simulate: per selected locus and per sample, one replicate GENEALOGY drawn from the structured coalescent
// with migration under the sampled parameters, G_rep ~ p(G | Theta_s), and the discrepancy of the sampled genealogy against it
// (include/gphocs_hip.h, gph_engine_simulate_*).  `--predictive` redraws the data on the sampled genealogy and so tests the
// mutation process alone; this is the part that confronts the demographic model.
//
// All arithmetic is plain uncontracted fp64 in the order written; log is gph_log; x / theta_p is the correctly rounded quotient
// (gph_quot with the chain state's RN(1 / theta_p)), every other quotient IEEE division.
//
// Generator.  mix = gph_pd_mix (gph_predictive.h).  Kl = mix((seed ^ GPH_SI_DOMAIN) ^ mix(g + 0x9E3779B97F4A7C15)) for the GLOBAL
// locus index g (host, at enable; GPH_SI_DOMAIN keeps the stream apart from --predictive's and from the site hashes), Ks =
// mix(Kl + t) for sample t, Ka = mix(Ks + (a + 1) GPH_SI_ATTEMPT) for attempt a = 0 .. 15, and draw d = 0, 1, ... of the attempt
// is u_d = ((mix(Ka ^ d) >> 12) + 0.5) 2^-52, in (0, 1).  A replicate is a pure function of (seed, g, t) and the model: it does
// not depend on lanes, ranks or the selection, and touches no page, no locus generator and no chain state.
//
// The simulation of one attempt, backwards in time.  The model: theta, popAge, sampleAge, popFather, migRate, bandStart, bandEnd,
// bandSrc, bandTgt of the chain state.  A LINEAGE is (node, population); the lineages stand in a list.
//   enter(t)   every current population p in index order that has not entered and has sampleAge[p] <= t enters: its leaves are
//              appended in leaf order, each in p (leaf i's record: age sampleAge[p], npop p).  Then every lineage in list order
//              climbs: while its population has a father F with popAge[F] <= t it moves to F.
//   start      t = 0, enter(0).
//   step       if one lineage is left and every population has entered: the end, the root is node N - 1.
//              c[p] = lineages in p.  Rates in this order: p = 0 .. K - 1 with c[p] >= 2: r = (c (c - 1)) / theta_p; then b = 0 ..
//              B - 1 with bandStart[b] <= t < bandEnd[b] and c[tgt b] >= 1: r = c[tgt b] migRate[b]; R = their sum in that order.
//              nb = the smallest of popAge[p] (p >= Kc), sampleAge[p] (p < Kc), bandStart[b], bandEnd[b] that is > t (none: inf).
//              u = the next draw (always spent), w = -log(u) / R.  If !(R > 0) or t + w >= nb: t' = nb, else t' = t + w.  t' = inf:
//              the attempt fails.  Exposure with dt = t' - t: coal_p += (c (c - 1)) dt for c[p] >= 2, mig_b += c[tgt b] dt for the
//              bands live at t with c >= 1.  t = t'.  At a boundary: enter(t), next step.  Else the next draw x = u R picks the
//              event: walking the non-zero rates in the same order with acc = acc + r, the first with x < acc; the last non-zero
//              rate takes the rounding residue.
//   coalescence in p, c = c[p]: a = min(int(u c), c - 1), b = min(int(u' (c - 1)), c - 2) from two further draws, b += (b >= a);
//              the a-th and b-th lineages of p in list order; node v = n + (coalescences so far): age t, npop p, left = the one
//              earlier in the list, right = the later; v takes the earlier slot, the later slot is removed, the order is kept.
//   migration in b: with GPH_MAX_MIGS migrations recorded already the attempt is ABANDONED (the chain's prior is truncated there:
//              rejecting is exact for it).  k = min(int(u c[tgt b]), c - 1) from one further draw; the k-th lineage of tgt b in
//              list order moves to bandSrc[b]; migration m = (migrations so far): branch = its node, band b, spop = bandSrc[b],
//              tpop = bandTgt[b], age t, living[m] = m.
// After GPH_SI_ATTEMPTS failed attempts the locus's replicate of that sample is FAILED: counted, and left out of every statistic.
//
// The replicate record has the layout of a --gene-trees record (gph_gt_shape); dataLnL = 0; genLnL is gtree_lnl (gph_locus.h) on
// the replicate's counts and exposures: lnL = 0; p = 0 .. K - 1: lnL += n_p logTwoTheta[p] - coal_p / theta_p; b = 0 .. B - 1 with
// migRate[b] > 0: lnL += m_b logMigRate[b] - mig_b migRate[b] -- every population and band, the terms the engine includes, no
// constant.  A failed replicate's record is all zero with root -1.  recs [nsel][record] holds the latest sample's replicates.
//
// Statistics, M = 3 + K + B: tmrca (the root's age), length (sum over non-root nodes v in node order of age[father v] - age[v]),
// genLnL, coal_p (coalescences in p), mig_b (migrations in b).  x = on the sampled genealogy (settled node records, the page's
// ncoal / nmig and FS_GENLNL), y = on the replicate.  Per (selected locus, statistic) five doubles: gt += (y > x), eq += (y == x),
// sx += x, sy += y, sy2 += y y; behind them one double, the failed replicates of the locus: W = 5 M + 1, each word owned by one
// lane.  The sample's row, 2 (K + B) + 4 u64 added with integer atomics: sampled coal_p, mig_b, replicate coal_p, mig_b, the loci
// with y > x for tmrca, length, genLnL, and `failed`.
//
// Shape.  The event loop of a locus is serial (about 2 n + migrations + boundaries steps of a few dozen instructions): ONE LANE
// PER LOCUS, the lineage list, the counts and the exposures in lane-owned LDS ([index][lane]: conflict-free), the model of the
// chain state once per workgroup in LDS.  The workgroup size is what GPH_SI_LDS_BUDGET leaves: 256 lanes while a lane's part stays
// under about 150 bytes, halved until it fits, 16 at least.  Node records go straight into the replicate record in HBM (a
// lane-owned record: a 16-byte store a node, a 2-byte store when it gets its father).
// The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane.
#pragma once
#include "gph_predictive.h"
#include "gph_genetrees.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 16

#define GPH_SI_MAXTHREADS 256
#define GPH_SI_LDS_BUDGET 40960
#define GPH_SI_ATTEMPTS 16
#define GPH_SI_DOMAIN 0x53494d554c415445ull       // "SIMULATE"
#define GPH_SI_ATTEMPT 0xd1b54a32d192ed03ull
#define GPH_SI_SITES 0x5349544553ull                // "SITES": the site level's Kl is gph_si_locus_key(seed ^ GPH_SI_SITES, g)
enum { SI_GT = 0, SI_EQ, SI_SX, SI_SY, SI_SY2, SI_WORDS };
enum { SI_TMRCA = 0, SI_LENGTH, SI_GENLNL, SI_FIXED };

struct GphSiShape {
  int32_t bd;                   // lanes of a workgroup = loci of a workgroup
  int32_t M, W, RC;             // statistics, doubles a locus (5 M + 1), columns of a row
  int32_t per_lane;             // bytes of LDS a lane owns
  int32_t o_sd, o_ld, o_s16, o_l16, o_s8, o_l8;   // byte offsets in the dynamic LDS: shared / lane-owned doubles, 16-bit, bytes
  int32_t lds_bytes;
};

GPH_SM_HD int32_t gph_si_stats(int K, int B) { return SI_FIXED + K + B; }

GPH_SM_HD void gph_si_shape(const GphLayout &y, GphSiShape &h)
{
  const int n = y.n > 0 ? y.n : 1, K = y.K > 0 ? y.K : 1, B = y.B > 0 ? y.B : 0;
  h.M = gph_si_stats(K, B); h.W = SI_WORDS * h.M + 1; h.RC = 2 * (K + B) + SI_FIXED + 1;
  h.per_lane = 8 * (K + B) + 2 * n + n + 2 * K + B;
  const int shared = 8 * (5 * K + 4 * B) + 2 * (K + 2 * B) + n + 32;
  int bd = GPH_SI_MAXTHREADS;
  while (bd > 16 && shared + bd * h.per_lane > GPH_SI_LDS_BUDGET) bd >>= 1;
  h.bd = bd;
  int at = 0;
  h.o_sd = at; at += 8 * (5 * K + 4 * B);
  h.o_ld = at; at += 8 * (K + B) * bd;
  h.o_s16 = at; at += 2 * (K + 2 * B);
  at = (at + 3) & ~3;
  h.o_l16 = at; at += 2 * n * bd;
  h.o_s8 = at; at += n;
  at = (at + 3) & ~3;
  h.o_l8 = at; at += (n + 2 * K + B) * bd;
  h.lds_bytes = (at + 15) & ~15;
}

struct GphSiLds {
  double *theta, *thetaInv, *logTwoTheta, *popAge, *sampleAge;    // [K] the chain state's
  double *migRate, *logMigRate, *bandStart, *bandEnd;             // [B]
  double *coalst, *migst;       // [K][bd], [B][bd] lane-owned: the exposures
  int16_t *popFather;           // [K]
  int16_t *bandSrc, *bandTgt;   // [B]
  int16_t *lnode;               // [n][bd] lane-owned: the node of a lineage
  uint8_t *leafpop;             // [n]
  uint8_t *lpop;                // [n][bd] lane-owned: the population of a lineage
  uint8_t *cnt, *ncoal;         // [K][bd] lane-owned: lineages in p, coalescences in p
  uint8_t *nmig;                // [B][bd] lane-owned: migrations in b
};
GPH_SM_FN void gph_si_carve(char *base, const GphLayout &y, const GphSiShape &h, GphSiLds &s)
{
  const int n = y.n, K = y.K, B = y.B, bd = h.bd;
  double *d = (double *)(base + h.o_sd);
  s.theta = d; s.thetaInv = d + K; s.logTwoTheta = d + 2 * K; s.popAge = d + 3 * K; s.sampleAge = d + 4 * K;
  d += 5 * K;
  s.migRate = d; s.logMigRate = d + B; s.bandStart = d + 2 * B; s.bandEnd = d + 3 * B;
  s.coalst = (double *)(base + h.o_ld); s.migst = s.coalst + K * bd;
  s.popFather = (int16_t *)(base + h.o_s16); s.bandSrc = s.popFather + K; s.bandTgt = s.bandSrc + B;
  s.lnode = (int16_t *)(base + h.o_l16);
  s.leafpop = (uint8_t *)(base + h.o_s8);
  s.lpop = (uint8_t *)(base + h.o_l8); s.cnt = s.lpop + n * bd; s.ncoal = s.cnt + K * bd; s.nmig = s.ncoal + K * bd;
}

// Kl of global locus g (host, at enable)
GPH_SM_HD uint64_t gph_si_locus_key(uint64_t seed, uint64_t g) { return gph_pd_locus_key(seed ^ GPH_SI_DOMAIN, g); }

// draw d of the attempt, in (0, 1); d moves on
GPH_SM_FN double gph_si_draw(uint64_t Ka, uint32_t &d)
{
  const uint64_t hv = gph_pd_mix(Ka ^ (uint64_t)d);
  d++;
  return ((double)(hv >> 12) + 0.5) * (1.0 / 4503599627370496.0);
}
// min(int(u c), c - 1)
GPH_SM_FN int gph_si_pick(double u, int c)
{
  const int k = (int)(u * (double)c);
  return k < c - 1 ? k : c - 1;
}

// lane-owned element i of an array of `cap` elements a lane
#define GPH_SI_AT(i, cap) GPH_IX((i) * bd + tid, (cap) * bd)

struct GphSiRun {               // one lane's attempt
  int len;                      // lineages in the list
  uint64_t entered;             // bit p: current population p has entered
  int nco, nm;                  // coalescences, migrations so far
};

GPH_SM_FN void gph_si_node(char *nodes, int N, int v, double age, int father, int left, int right, int npop)
{
  alignas(16) GphNode rec;
  rec.age = age; rec.father = (int16_t)father; rec.left = (int16_t)left; rec.right = (int16_t)right; rec.npop = (int16_t)npop;
  gph_copy16(nodes + (size_t)GPH_IX(v, N) * 16, &rec);
}

// enter(t)
GPH_SM_FN void gph_si_enter(const GphSiLds &s, const GphLayout &y, int bd, int tid, double t, GphSiRun &r, char *nodes)
{
  const int n = y.n, N = y.N, K = y.K, Kc = y.Kc;
  for (int p = 0; p < Kc; p++) {
    if ((r.entered >> p) & 1u) continue;
    const double sa = s.sampleAge[GPH_IX(p, K)];
    if (!(sa <= t)) continue;
    r.entered |= (uint64_t)1 << p;
    for (int i = 0; i < n; i++) {
      if (s.leafpop[GPH_IX(i, n)] != p || r.len >= n) continue;
      s.lnode[GPH_SI_AT(r.len, n)] = (int16_t)i;
      s.lpop[GPH_SI_AT(r.len, n)] = (uint8_t)p;
      s.cnt[GPH_SI_AT(p, K)]++;
      r.len++;
      gph_si_node(nodes, N, i, sa, -1, -1, -1, p);
    }
  }
  for (int k = 0; k < r.len; k++) {
    int q = s.lpop[GPH_SI_AT(k, n)];
    for (int guard = 0; guard < K; guard++) {
      const int F = (unsigned)q < (unsigned)K ? s.popFather[GPH_IX(q, K)] : -1;
      if ((unsigned)F >= (unsigned)K || !(s.popAge[GPH_IX(F, K)] <= t)) break;
      s.cnt[GPH_SI_AT(q, K)]--;
      s.cnt[GPH_SI_AT(F, K)]++;
      q = F;
    }
    s.lpop[GPH_SI_AT(k, n)] = (uint8_t)q;
  }
}

// the list position of the k-th lineage of population p (list order); -1: there is none
GPH_SM_FN int gph_si_kth(const GphSiLds &s, int n, int bd, int tid, int len, int p, int k)
{
  for (int i = 0; i < len; i++)
    if (s.lpop[GPH_SI_AT(i, n)] == p && k-- == 0) return i;
  return -1;
}

// rate idx of the walk: populations 0 .. K - 1, then bands K .. K + B - 1; 0 where there is none
GPH_SM_FN double gph_si_rate(const GphSiLds &s, int K, int B, int bd, int tid, double t, int idx, int &c)
{
  if (idx < K) {
    c = s.cnt[GPH_SI_AT(idx, K)];
    if (c < 2) return 0.0;
    return gph_quot((double)(c * (c - 1)), s.theta[GPH_IX(idx, K)], s.thetaInv[GPH_IX(idx, K)]);
  }
  const int b = idx - K, tgt = s.bandTgt[GPH_IX(b, B)];
  c = 0;
  if (!(s.bandStart[GPH_IX(b, B)] <= t && t < s.bandEnd[GPH_IX(b, B)]) || (unsigned)tgt >= (unsigned)K) return 0.0;
  c = s.cnt[GPH_SI_AT(tgt, K)];
  if (c < 1) return 0.0;
  return (double)c * s.migRate[GPH_IX(b, B)];
}

// one attempt of lane tid into the record; 0: a genealogy, 1: abandoned at the migration cap, 2: no way on (a damaged model)
GPH_SM_FN int gph_si_attempt(const GphSiLds &s, const GphLayout &y, const GphGtShape &gs, int bd, int tid, uint64_t Ka, char *rec, GphSiRun &r)
{
  const int n = y.n, N = y.N, K = y.K, Kc = y.Kc, B = y.B;
  char *nodes = rec + gs.off[GT_O_NODES];
  uint32_t d = 0;
  r.len = 0; r.entered = 0; r.nco = 0; r.nm = 0;
  const uint64_t all = Kc >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << Kc) - 1);
  for (int p = 0; p < K; p++) { s.cnt[GPH_SI_AT(p, K)] = 0; s.ncoal[GPH_SI_AT(p, K)] = 0; s.coalst[GPH_SI_AT(p, K)] = 0.0; }
  for (int b = 0; b < B; b++) { s.nmig[GPH_SI_AT(b, B)] = 0; s.migst[GPH_SI_AT(b, B)] = 0.0; }
  double t = 0.0;
  gph_si_enter(s, y, bd, tid, t, r, nodes);
  const int maxsteps = n + GPH_MAX_MIGS + K + Kc + 2 * B + 8;
  for (int step = 0; step < maxsteps; step++) {
    if (r.len == 1 && r.entered == all) return 0;
    double R = 0.0;
    int c;
    for (int idx = 0; idx < K + B; idx++) {
      const double rt = gph_si_rate(s, K, B, bd, tid, t, idx, c);
      if (rt != 0.0) R = R + rt;
    }
    double nb = (double)INFINITY;
    for (int p = 0; p < K; p++) {
      const double a = p < Kc ? s.sampleAge[GPH_IX(p, K)] : s.popAge[GPH_IX(p, K)];
      if (a > t && a < nb) nb = a;
    }
    for (int b = 0; b < B; b++) {
      const double a0 = s.bandStart[GPH_IX(b, B)], a1 = s.bandEnd[GPH_IX(b, B)];
      if (a0 > t && a0 < nb) nb = a0;
      if (a1 > t && a1 < nb) nb = a1;
    }
    const double u = gph_si_draw(Ka, d);
    const double w = -gph_log(u) / R;
    const bool jump = !(R > 0.0) || t + w >= nb;
    const double tn = jump ? nb : t + w;
    if (!(tn < (double)INFINITY)) return 2;
    const double dt = tn - t;
    for (int idx = 0; idx < K + B; idx++) {
      const double rt = gph_si_rate(s, K, B, bd, tid, t, idx, c);
      if (rt == 0.0) continue;
      if (idx < K) s.coalst[GPH_SI_AT(idx, K)] = s.coalst[GPH_SI_AT(idx, K)] + (double)(c * (c - 1)) * dt;
      else s.migst[GPH_SI_AT(idx - K, B)] = s.migst[GPH_SI_AT(idx - K, B)] + (double)c * dt;
    }
    const double t0 = t;
    t = tn;
    if (jump) { gph_si_enter(s, y, bd, tid, t, r, nodes); continue; }
    const double x = gph_si_draw(Ka, d) * R;
    double acc = 0.0;
    int chosen = -1, last = -1;
    for (int idx = 0; idx < K + B; idx++) {
      const double rt = gph_si_rate(s, K, B, bd, tid, t0, idx, c);
      if (rt == 0.0) continue;
      last = idx;
      acc = acc + rt;
      if (chosen < 0 && x < acc) chosen = idx;
    }
    if (chosen < 0) chosen = last;
    if (chosen < 0) return 2;
    if (chosen < K) {
      const int p = chosen, cp = s.cnt[GPH_SI_AT(p, K)];
      const int a = gph_si_pick(gph_si_draw(Ka, d), cp);
      int b = gph_si_pick(gph_si_draw(Ka, d), cp - 1);
      if (b >= a) b++;
      const int klo = gph_si_kth(s, n, bd, tid, r.len, p, a < b ? a : b), khi = gph_si_kth(s, n, bd, tid, r.len, p, a < b ? b : a);
      const int v = n + r.nco;
      if (klo < 0 || khi < 0 || v >= N) return 2;
      const int left = s.lnode[GPH_SI_AT(klo, n)], right = s.lnode[GPH_SI_AT(khi, n)];
      gph_si_node(nodes, N, v, t, -1, left, right, p);
      *(int16_t *)(nodes + (size_t)GPH_IX(left, N) * 16 + 8) = (int16_t)v;
      *(int16_t *)(nodes + (size_t)GPH_IX(right, N) * 16 + 8) = (int16_t)v;
      s.lnode[GPH_SI_AT(klo, n)] = (int16_t)v;
      for (int k = khi; k + 1 < r.len; k++) {
        s.lnode[GPH_SI_AT(k, n)] = s.lnode[GPH_SI_AT(k + 1, n)];
        s.lpop[GPH_SI_AT(k, n)] = s.lpop[GPH_SI_AT(k + 1, n)];
      }
      r.len--;
      s.cnt[GPH_SI_AT(p, K)]--;
      s.ncoal[GPH_SI_AT(p, K)]++;
      r.nco++;
    } else {
      const int b = chosen - K, tgt = s.bandTgt[GPH_IX(b, B)], src = s.bandSrc[GPH_IX(b, B)];
      if (r.nm >= GPH_MAX_MIGS) return 1;
      if ((unsigned)src >= (unsigned)K) return 2;
      const int k = gph_si_kth(s, n, bd, tid, r.len, tgt, gph_si_pick(gph_si_draw(Ka, d), (int)s.cnt[GPH_SI_AT(tgt, K)]));
      if (k < 0) return 2;
      const int m = r.nm;
      ((double *)(rec + gs.off[GT_O_MIG_AGE]))[GPH_IX(m, GPH_MAX_MIGS)] = t;
      int16_t *mi = (int16_t *)(rec + gs.off[GT_O_MIG_I]) + GPH_IX(m, GPH_MAX_MIGS) * MG_COUNT;
      mi[MG_BRANCH] = s.lnode[GPH_SI_AT(k, n)]; mi[MG_BAND] = (int16_t)b; mi[MG_SPOP] = (int16_t)src; mi[MG_TPOP] = (int16_t)tgt;
      mi[MG_SEV] = -1; mi[MG_TEV] = -1;
      ((int16_t *)(rec + gs.off[GT_O_LIVING]))[GPH_IX(m, GPH_MAX_MIGS)] = (int16_t)m;
      s.lpop[GPH_SI_AT(k, n)] = (uint8_t)src;
      s.cnt[GPH_SI_AT(tgt, K)]--;
      s.cnt[GPH_SI_AT(src, K)]++;
      s.nmig[GPH_SI_AT(b, B)]++;
      r.nm++;
    }
  }
  return r.len == 1 && r.entered == all ? 0 : 2;
}

// one statistic of one locus: x on the sampled genealogy, y on the replicate
GPH_SM_FN bool gph_si_update(double *a, double x, double yv)
{
  if (yv > x) a[SI_GT] = a[SI_GT] + 1.0;
  if (yv == x) a[SI_EQ] = a[SI_EQ] + 1.0;
  a[SI_SX] = a[SI_SX] + x;
  a[SI_SY] = a[SI_SY] + yv;
  a[SI_SY2] = a[SI_SY2] + yv * yv;
  return yv > x;
}

// sum over the nodes v != root, in node order, of age[father v] - age[v] (a father outside 0 .. N - 1 adds nothing)
GPH_SM_FN double gph_si_length(const char *nodes, int N, int root)
{
  double len = 0.0;
  for (int v = 0; v < N; v++) {
    if (v == root) continue;
    const GphNode *nd = (const GphNode *)(nodes + (size_t)v * 16);
    const int f = nd->father;
    if ((unsigned)f >= (unsigned)N) continue;
    len = len + (((const GphNode *)(nodes + (size_t)f * 16))->age - nd->age);
  }
  return len;
}

GPH_SM_FN void gph_si_clear(char *rec, int bytes)
{
  alignas(16) const uint64_t zero[2] = {0, 0};
  for (int o = 0; o < bytes; o += 16) gph_copy16(rec + o, zero);
}

// lane tid of workgroup bx = selected locus bx bd + tid, sample t.  key: Kl per selected locus; pop: leaf -> population;
// acc [nsel][W]; recs [nsel][record]; row [RC]
GPH_FLAT(k_simulate, GPH_SI_MAXTHREADS, GphKargs KA, GphSiShape h, GphGtShape gs, const char *pages, const int32_t *sel_slot, const uint64_t *key,
         const uint8_t *pop, int nsel, int L, long long t, double *acc, char *recs, uint64_t *row)
{
  GPH_FLAT_BODY(GphNoLane);
  const GphLayout &y = KA.lay;
  const GphModel &model = KA.G->model;
  const int n = y.n, N = y.N, K = y.K, B = y.B;
  GphSiLds s;
  gph_si_carve(lds, y, h, s);
  GPH_PHASE {
    for (int p = tid; p < K; p += bd) {
      s.theta[GPH_IX(p, K)] = model.theta[p]; s.thetaInv[GPH_IX(p, K)] = model.thetaInv[p]; s.logTwoTheta[GPH_IX(p, K)] = model.logTwoTheta[p];
      s.popAge[GPH_IX(p, K)] = model.popAge[p]; s.sampleAge[GPH_IX(p, K)] = model.sampleAge[p];
      s.popFather[GPH_IX(p, K)] = (int16_t)model.popFather[p];
    }
    for (int b = tid; b < B; b += bd) {
      s.migRate[GPH_IX(b, B)] = model.migRate[b]; s.logMigRate[GPH_IX(b, B)] = model.logMigRate[b];
      s.bandStart[GPH_IX(b, B)] = model.bandStart[b]; s.bandEnd[GPH_IX(b, B)] = model.bandEnd[b];
      s.bandSrc[GPH_IX(b, B)] = (int16_t)model.bandSrc[b]; s.bandTgt[GPH_IX(b, B)] = (int16_t)model.bandTgt[b];
    }
    for (int i = tid; i < n; i += bd) s.leafpop[GPH_IX(i, n)] = pop[GPH_IX(i, n)];
  }
  GPH_BARRIER;
  GPH_PHASE {
    const int q = bx * bd + tid;
    if (q < nsel) {
      const int j = GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
      const char *pg = pages + (size_t)j * y.page_bytes;
      char *rec = recs + (size_t)q * gs.img.bytes;
      double *a = acc + (size_t)q * h.W;
      const uint64_t Ks = gph_pd_mix(key[GPH_IX(q, nsel)] + (uint64_t)t);
      GphSiRun r;
      bool ok = false;
      gph_si_clear(rec, gs.img.bytes);
      for (int att = 0; att < GPH_SI_ATTEMPTS && !ok; att++)
        ok = gph_si_attempt(s, y, gs, bd, tid, gph_pd_mix(Ks + (uint64_t)(att + 1) * GPH_SI_ATTEMPT), rec, r) == 0;
      if (!ok) {
        gph_si_clear(rec, gs.img.bytes);
        *(int32_t *)(rec + gs.off[GT_O_ROOT]) = -1;
        a[GPH_IX(SI_WORDS * h.M, h.W)] = a[GPH_IX(SI_WORDS * h.M, h.W)] + 1.0;
        gph_lanes_add64(row + GPH_IX(h.RC - 1, h.RC), 1);
      } else {
        /* the migrations an abandoned attempt left behind those of this one */
        for (int m = r.nm; m < GPH_MAX_MIGS; m++) {
          ((double *)(rec + gs.off[GT_O_MIG_AGE]))[m] = 0.0;
          for (int k = 0; k < MG_COUNT; k++) ((int16_t *)(rec + gs.off[GT_O_MIG_I]))[m * MG_COUNT + k] = 0;
          ((int16_t *)(rec + gs.off[GT_O_LIVING]))[m] = 0;
        }
        double lnl = 0.0;
        for (int p = 0; p < K; p++)
          lnl += (double)s.ncoal[GPH_SI_AT(p, K)] * s.logTwoTheta[GPH_IX(p, K)] -
                 gph_quot(s.coalst[GPH_SI_AT(p, K)], s.theta[GPH_IX(p, K)], s.thetaInv[GPH_IX(p, K)]);
        for (int b = 0; b < B; b++) {
          const double rate = s.migRate[GPH_IX(b, B)];
          if (rate > 0.0) lnl += (double)s.nmig[GPH_SI_AT(b, B)] * s.logMigRate[GPH_IX(b, B)] - s.migst[GPH_SI_AT(b, B)] * rate;
        }
        const int root = N - 1;
        *(int32_t *)(rec + gs.off[GT_O_ROOT]) = root;
        *(int32_t *)(rec + gs.off[GT_O_NUM_MIGS]) = r.nm;
        *(double *)(rec + gs.off[GT_O_DATALNL]) = 0.0;
        *(double *)(rec + gs.off[GT_O_GENLNL]) = lnl;
        const char *rnodes = rec + gs.off[GT_O_NODES];
        /* the sampled genealogy: the page */
        const int32_t *is = (const int32_t *)(pg + y.o_iscal);
        const int sroot = (unsigned)is[IS_ROOT] < (unsigned)N ? is[IS_ROOT] : 0;      /* (a damaged page must not reach past the records) */
        const char *snodes = pg + y.o_nd;
        const int16_t *sncoal = (const int16_t *)(pg + y.o_ncoal), *snmig = (const int16_t *)(pg + y.o_nmig);
        if (gph_si_update(a + SI_WORDS * SI_TMRCA, ((const GphNode *)(snodes + (size_t)sroot * 16))->age, ((const GphNode *)(rnodes + (size_t)root * 16))->age))
          gph_lanes_add64(row + GPH_IX(2 * (K + B) + SI_TMRCA, h.RC), 1);
        if (gph_si_update(a + SI_WORDS * SI_LENGTH, gph_si_length(snodes, N, sroot), gph_si_length(rnodes, N, root)))
          gph_lanes_add64(row + GPH_IX(2 * (K + B) + SI_LENGTH, h.RC), 1);
        if (gph_si_update(a + SI_WORDS * SI_GENLNL, ((const double *)(pg + y.o_fscal))[FS_GENLNL], lnl))
          gph_lanes_add64(row + GPH_IX(2 * (K + B) + SI_GENLNL, h.RC), 1);
        for (int c = 0; c < K + B; c++) {
          const int xs = c < K ? sncoal[c] : snmig[c - K];
          const int ys = c < K ? s.ncoal[GPH_SI_AT(c, K)] : s.nmig[GPH_SI_AT(c - K, B)];
          (void)gph_si_update(a + (size_t)SI_WORDS * GPH_IX(SI_FIXED + c, h.M), (double)xs, (double)ys);
          if (xs > 0) gph_lanes_add64(row + GPH_IX(c, h.RC), (uint64_t)xs);
          if (ys > 0) gph_lanes_add64(row + GPH_IX(K + B + c, h.RC), (uint64_t)ys);
        }
      }
    }
  }
}

#undef GPH_SI_AT
#undef GPH_FILE_ID
#define GPH_FILE_ID 2
