// gph_mutations.h -- k_mutations: the posterior expected number of substitutions inside each population and on each sample's
// terminal branch, given the data and the sampled genealogy, next to what the one clock expects on the same exposure; per
// selected locus and genome-wide per sample, on the device (include/gphocs_hip.h, gph_engine_mutations_*).
//
// Definitions (include/gphocs_hip.h has them in full).  All arithmetic is plain uncontracted fp64 in the order written, exp is
// gph_exp, a quotient is IEEE division.  One locus at one sample: n leaves, N = 2n - 1 nodes, rows 0 .. P - 1 of its sequence
// block; a COLUMN is a row with a non-zero phase word with the ph - 1 rows behind it and stands for `count` sites
// (gph_predictive.h); sites = sum count; rate = FS_MUTRATE.
//   Branch above v != root, father f: t_v = age[f] - age[v], len = rate t_v, a = 4 len / 3.0, u = len < 1e-100 ? 0 :
//   1 - exp(-4 len / 3.0), pe = u / 4.0, qe = 1 - 4.0 pe (edge_prob and the likelihood's qe),
//     E_diff = (a qe) / u + 0.75 a      expected substitutions of a JC69 path whose ends differ (uniformisation: exact)
//     E_same = ((0.75 a) u) / (1 + 3 qe)                                          ... whose ends are equal
//   u == 0: the branch contributes nothing (M_v = 0, no segment).
//   Per row.  I_v: the inside conditional of v -- an internal node's CURRENT half (IS_CBIT) where it lies in the conditional
//   arrays, a leaf's one-hot vector (all ones for code 4).  Top down: O_root(x) = 1.0; for a child c of v with sibling s
//   U_c(x) = O_v(x) f_s(x), f_s = child_factor of the sibling as the likelihood forms it (S >= 4 -> 1.0 included);
//   SU = ((U_c(0) + U_c(1)) + U_c(2)) + U_c(3); O_c(y) = pe_c SU + qe_c U_c(y).  J_x = the sum of I_c(y), y != x, y increasing;
//     D_c(row) = pe_c (((U_c(0) J_0 + U_c(1) J_1) + U_c(2) J_2) + U_c(3) J_3)      the mass of "the ends of c's branch differ"
//     R(row) = ((r0 + r1) + r2) + r3 of the root's conditionals
//   Per column j: DD = sum D, RR = sum R over its rows in row order, d = RR == 0 ? 0 : DD / RR; Dv = sum_j (double)count_j d in
//   column order; M_v = E_same (sites - Dv) + E_diff Dv.
//   Segments of the branch above v: cur = npop[v], t = age[v]; the events are the live migrations whose branch is v by increasing
//   age (equal ages in `living` order), then age[f].  Before an event at age b: while cur has a father population F with
//   popAge[F] <= b, close (cur, popAge[F] - t), cur = F, t = popAge[F]; then close (cur, b - t), t = b, and at a migration
//   cur = bandSrc[its band].  Segment (p, dt): mut_p = mut_p + M_v (dt / t_v), exp_p = exp_p + (rate dt) sites; nodes in index
//   order, segments in time order.  Leaf i: mutExt_i = M_i, expExt_i = (rate t_i) sites.
// Columns, C = 2 (K + n): mut_p [K], exp_p [K], mutExt_i [n], expExt_i [n].
// Kept: per selected locus C doubles, acc = acc + value a sample by the one lane that owns the word; per sample one row, the
// selected loci added in selection order inside a chunk of GPH_MU_CHUNK loci (one workgroup, one partial row) and the partial
// rows in chunk order by k_rows_fold (gph_sampler.h) -- no fp atomics: a row is rebuilt bit for bit.
//
// Shape.  Workgroup w takes the chunk of selected loci w GPH_MU_CHUNK ..., one after the other, 64 lanes.
//   stage    the N node records with 128-bit loads, mig_age / mig_i / living, the current-half bit of every node; a lane a node
//            forms pe, qe; one lane lists the internal nodes father-first (a breadth-first walk from the root, at most n - 1
//            entries whatever the record holds).  popAge, popFather and bandSrc of the chain state go into LDS once a workgroup.
//   rows     the rows of the locus go on the lanes in TILES of TR rows -- every locus, P > TR and blocks the sweep keeps in HBM
//            included: the block is read where it lies.  A tile is STAGED first: the current half of every internal node's
//            conditionals goes from HBM into that node's PARKING SLOT (32 bytes a node and row, 16-byte units on consecutive
//            lanes), the code nibbles, phase words and counts next to it -- every load of the tile in flight at once.  Then a
//            lane walks the list once, LDS and registers only: I_c of a child comes from c's slot or the codes, O_v from v's
//            slot; O_c of an internal child goes into c's slot -- I_c has just been consumed --, and v's slot, dead from there
//            on, takes D of its two children.  The parking is (n - 1) slots of 4 doubles a row, [slot][x][row]
//            (conflict-free); TR = the rows that fit GPH_MU_LDS_BUDGET = 40 KB next to the rest, at most GPH_MU_TILE = 32 and at
//            most Pmax: 32 at 16 leaves, 28 at 32, 7 at 72, 3 at 136, 1 at 180.  Beyond 180 leaves one row no longer fits the
//            budget and gph_engine_mutations_enable refuses.  No register stack (its depth would be the tree's: n - 1 for a
//            caterpillar), no HBM scratch.
//   columns  a lane a branch walks the tile's rows in row order and keeps DD, RR, the open column's count, Dv and the sites in
//            LDS across tiles: a column longer than a tile keeps its row-order sums.
//   close    a lane a branch closes the last column and forms M_v, then walks the segments of ITS branch once and lists them
//            with their two terms (GPH_MU_SEGS = 4 entries a branch in LDS); then lane p < K adds, nodes in index order, what
//            the lists hold for ITS population (a branch with more segments than its list holds is walked again by that lane:
//            same arithmetic, same order), lane K + i takes leaf i; each adds its values to the locus's accumulators and to
//            the chunk's partial row (LDS, lane-owned words).  Where the lists do not fit next to a tile of 4 rows (about 120
//            leaves and more) there are none, and every population lane walks every branch.
// LDS: 16 N (records) + 16 N (pe, qe) + 48 N (column state, M) + 74 N (segment lists) + 14 TR + 8 C + 32 (n - 1) TR + 10 K + 2 B + 256.
// The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// It writes no page, draws no random number and touches no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 15

#define GPH_MU_THREADS 64
#define GPH_MU_CHUNK 64          // selected loci a workgroup and partial row (the fold adds the partial rows one after the other)
#define GPH_MU_TILE 32           // rows of a tile at most: the parking of 16 leaves is then 15 KB, 21.7 KB a workgroup, 7 of them a CU
#define GPH_MU_SEGS 4            // segments a branch's list holds: a branch with more (migrations, several taus) is walked again
#define GPH_MU_LDS_BUDGET 40960
enum { MU_DD = 0, MU_RR, MU_DV, MU_CNT, MU_SITES, MU_M, MU_WORDS };

struct GphMuShape {
  int32_t bd, TR, chunk, C;     // lanes, rows of a tile, selected loci a workgroup, columns
  int32_t segcap;               // segments a branch's list holds (0: no lists, every population walks every branch)
  int32_t o_nd, o_pe, o_qe, o_car, o_prow, o_mage, o_mpa, o_R, o_segm, o_segx, o_cnt, o_migi, o_ord, o_ph, o_mpf, o_segn, o_segp, o_cb, o_codes, o_park;   // byte offsets in the dynamic LDS
  int32_t lds_bytes;
};

GPH_SM_HD int32_t gph_mu_columns(int n, int K) { return 2 * (K + n); }

GPH_SM_HD void gph_mu_shape(const GphLayout &y, GphMuShape &h)
{
  const int n = y.n > 1 ? y.n : 2, N = 2 * n - 1, K = y.K > 0 ? y.K : 1, B = y.B > 0 ? y.B : 0;
  h.bd = GPH_MU_THREADS; h.chunk = GPH_MU_CHUNK; h.C = gph_mu_columns(n, K);
  int fixed = 16 * N + 8 * N + 8 * N + 8 * MU_WORDS * N + 8 * h.C + 8 * GPH_MAX_MIGS + 8 * K + 2 * (K + B) + 4 * N +
              ((2 * GPH_MAX_MIGS * (MG_COUNT + 1) + 2 * n + 15) & ~15) + 32;
  /* the segment lists, GPH_MU_SEGS entries a branch, where they leave room for a tile of 4 rows at least */
  const int per_row = 32 * (n - 1) + 14 + GPH_Q_NH(n);
  const int cap = fixed + 18 * GPH_MU_SEGS * N + 4 * per_row <= GPH_MU_LDS_BUDGET ? GPH_MU_SEGS : 0;
  h.segcap = cap;
  fixed += 18 * cap * N;
  int tr = (GPH_MU_LDS_BUDGET - fixed) / per_row;
  if (tr > GPH_MU_TILE) tr = GPH_MU_TILE;
  if (y.Pmax > 0 && tr > y.Pmax) tr = y.Pmax;
  if (tr < 1) tr = 1;
  h.TR = tr;
  int at = 0;
  h.o_nd = at; at += 16 * N;
  h.o_pe = at; at += 8 * N;
  h.o_qe = at; at += 8 * N;
  h.o_car = at; at += 8 * MU_WORDS * N;
  h.o_prow = at; at += 8 * h.C;
  h.o_mage = at; at += 8 * GPH_MAX_MIGS;
  h.o_mpa = at; at += 8 * K;
  h.o_segm = at; at += 8 * cap * N;
  h.o_segx = at; at += 8 * cap * N;
  h.o_R = at; at += 8 * tr;
  h.o_park = at; at += 32 * (n - 1) * tr;
  h.o_cnt = at; at += 4 * tr;
  h.o_migi = at; at += 2 * GPH_MAX_MIGS * (MG_COUNT + 1);     /* mig_i, then living */
  h.o_ord = at; at += 2 * n;                                  /* [0] entries, then the list */
  h.o_ph = at; at += 2 * tr;
  h.o_mpf = at; at += 2 * (K + B);
  h.o_segn = at; at += 2 * N;
  h.o_segp = at; at += 2 * cap * N;
  h.o_cb = at; at += 2 * N;
  h.o_codes = at; at += tr * GPH_Q_NH(n);
  h.lds_bytes = (at + 15) & ~15;
}

struct GphMuLds {
  GphNode *nd;          // [N]
  double *pe, *qe;      // [N] by child node; the root and a branch with u == 0: pe 0
  double *car;          // [MU_WORDS][N] column state of every branch, then M_v
  double *prow;         // [C] the chunk's partial row
  double *mage;         // [GPH_MAX_MIGS]
  double *mpa;          // [K] popAge of the chain state
  double *segm, *segx;  // [N][segcap] the terms of a branch's segments: M_v (dt / t_v), (rate dt) sites
  double *R;            // [TR]
  double *park;         // [n - 1][4][TR]
  int32_t *cnt;         // [TR] count of the row
  int16_t *migi;        // [GPH_MAX_MIGS][MG_COUNT], then living [GPH_MAX_MIGS]
  int16_t *ord;         // [0]: entries, [1 ..]: the internal nodes, father first
  uint16_t *ph;         // [TR] phase word of the row
  int16_t *mpf;         // [K] popFather, then [B] bandSrc, of the chain state
  int16_t *segn;        // [N] segments of the branch (may exceed segcap: then the list is not used)
  int16_t *segp;        // [N][segcap] population of a segment
  int16_t *cb;          // [N] which half of the conditional arrays is a node's current one
  uint8_t *codes;       // [TR][NH] the tile's code nibbles
};
GPH_SM_FN void gph_mu_carve(char *b, const GphMuShape &h, GphMuLds &s)
{
  s.nd = (GphNode *)(b + h.o_nd); s.pe = (double *)(b + h.o_pe); s.qe = (double *)(b + h.o_qe); s.car = (double *)(b + h.o_car);
  s.prow = (double *)(b + h.o_prow); s.mage = (double *)(b + h.o_mage); s.R = (double *)(b + h.o_R);
  s.park = (double *)(b + h.o_park); s.cnt = (int32_t *)(b + h.o_cnt); s.migi = (int16_t *)(b + h.o_migi); s.ord = (int16_t *)(b + h.o_ord);
  s.ph = (uint16_t *)(b + h.o_ph);
  s.mpa = (double *)(b + h.o_mpa); s.segm = (double *)(b + h.o_segm); s.segx = (double *)(b + h.o_segx);
  s.mpf = (int16_t *)(b + h.o_mpf); s.segn = (int16_t *)(b + h.o_segn); s.segp = (int16_t *)(b + h.o_segp);
  s.cb = (int16_t *)(b + h.o_cb); s.codes = (uint8_t *)(b + h.o_codes);
}

// the father of v when the branch above v exists: an internal node other than v
GPH_SM_FN int gph_mu_father(const GphMuLds &s, int n, int N, int v)
{
  const int f = s.nd[GPH_IX(v, N)].father;
  return f >= n && f < N && f != v ? f : -1;
}

// pe, qe of the branch above v (0, 1 where there is none or u == 0)
GPH_SM_FN void gph_mu_edge(const GphMuLds &s, int n, int N, int v, double rate)
{
  double pe = 0.0;
  const int f = gph_mu_father(s, n, N, v);
  if (f >= 0) {
    const double len = rate * (s.nd[GPH_IX(f, N)].age - s.nd[GPH_IX(v, N)].age);
    if (!(len < 1e-100)) {
      const double u = 1 - gph_exp(gph_quot(-4 * len, 3.0, 1.0 / 3.0));
      if (u > 0.0) pe = u / 4.0;                    /* (a NaN from a damaged record: no branch) */
    }
  }
  s.pe[GPH_IX(v, N)] = pe;
  s.qe[GPH_IX(v, N)] = 1 - 4.0 * pe;
}

// the internal nodes, father first: breadth-first from the root; n - 1 entries at most whatever the record holds
GPH_SM_FN void gph_mu_order(const GphMuLds &s, int n, int N, int root)
{
  int nord = 0;
  if (root >= n && root < N) s.ord[GPH_IX(1 + nord++, n)] = (int16_t)root;
  for (int k = 0; k < nord; k++) {
    const int v = s.ord[GPH_IX(1 + k, n)];
    const int l = s.nd[GPH_IX(v, N)].left, r = s.nd[GPH_IX(v, N)].right;
    if (l >= n && l < N && nord < n - 1) s.ord[GPH_IX(1 + nord++, n)] = (int16_t)l;
    if (r >= n && r < N && nord < n - 1) s.ord[GPH_IX(1 + nord++, n)] = (int16_t)r;
  }
  s.ord[0] = (int16_t)nord;
}

// I_c of child c at the tile's row `lane` into i[4]: a leaf's code, or what c's parking slot holds -- before c's father is
// walked that is the current half of c's conditionals, staged there by gph_mu_stage_tile
GPH_SM_FN void gph_mu_inside(const GphMuLds &s, int n, int TR, int lane, int c, double *i)
{
  if (c < n) {
    const int NH = GPH_Q_NH(n), code = (s.codes[GPH_IX(lane * NH + (c >> 1), TR * NH)] >> ((c & 1) << 2)) & 15;
    for (int x = 0; x < 4; x++) i[x] = code == 4 || code == x ? 1.0 : 0.0;
  } else {
    for (int x = 0; x < 4; x++) i[x] = s.park[GPH_IX((c - n) * 4 * TR + x * TR + lane, 4 * (n - 1) * TR)];
  }
}

// the tile's rows r0 .. r0 + rows - 1 from HBM into LDS, every load of the tile in flight at once: the current half of every
// internal node's conditionals into the node's parking slot (16 bytes a unit, consecutive lanes on consecutive units of a node:
// 32 bytes a row), the leaf codes, phase words and counts
GPH_SM_FN void gph_mu_stage_tile(const GphMuLds &s, const GphLayout &y, const GphMuShape &h, const char *blk, const double *cond, int P, int r0, int rows,
                                 int tid, int bd)
{
  const int n = y.n, TR = h.TR, NH = GPH_Q_NH(n), per = 2 * rows, slots = 4 * (n - 1) * TR;
  const int q_phases = GPH_Q_PHASES(P, n), q_count = GPH_Q_COUNT(P, n);
  for (int u = tid; u < (n - 1) * per; u += bd) {
    const int k = u / per, w = u - k * per, row = w >> 1, x0 = (w & 1) << 1;
    const int half = s.cb[GPH_IX(n + k, y.N)];
    alignas(16) double two[2];
    gph_copy16(two, cond + ((size_t)(half * (n - 1) + k) * P + (size_t)GPH_IX(r0 + row, P)) * 4 + x0);
    s.park[GPH_IX((k * 4 + x0) * TR + row, slots)] = two[0];
    s.park[GPH_IX((k * 4 + x0 + 1) * TR + row, slots)] = two[1];
  }
  for (int b = tid; b < rows * NH; b += bd) s.codes[GPH_IX(b, TR * NH)] = ((const uint8_t *)blk)[GPH_Q_LEAF + (size_t)r0 * NH + b];
  for (int lane = tid; lane < rows; lane += bd) {
    const int r = r0 + lane;
    const uint16_t w = ((const uint16_t *)(blk + q_phases))[GPH_IX(r, P)];
    s.ph[GPH_IX(lane, TR)] = w;
    s.cnt[GPH_IX(lane, TR)] = w == 0 ? 0 : y.cnt16 ? (int32_t)((const uint16_t *)(blk + q_count))[GPH_IX(r, P)] : ((const int32_t *)(blk + q_count))[GPH_IX(r, P)];
    s.R[GPH_IX(lane, TR)] = 0.0;
  }
}

// child_factor of a child with inside vector i, for the four bases
GPH_SM_FN void gph_mu_factor(const double *i, double pe, double qe, double *f)
{
  double S = 0.0;
  S += i[0]; S += i[1]; S += i[2]; S += i[3];
  if (S >= 4) { f[0] = f[1] = f[2] = f[3] = 1.0; return; }
  const double Sp = S * pe;
  for (int x = 0; x < 4; x++) f[x] = Sp + i[x] * qe;
}

// the branch above child c of v at one row: U_c = O_v f_s; returns D_c, and O_c into o[4]
GPH_SM_FN double gph_mu_down(const double *O, const double *fs, const double *ic, double pe, double qe, double *o)
{
  double U[4];
  for (int x = 0; x < 4; x++) U[x] = O[x] * fs[x];
  const double SU = ((U[0] + U[1]) + U[2]) + U[3], pS = pe * SU;
  for (int x = 0; x < 4; x++) o[x] = pS + qe * U[x];
  const double J0 = (ic[1] + ic[2]) + ic[3], J1 = (ic[0] + ic[2]) + ic[3], J2 = (ic[0] + ic[1]) + ic[3], J3 = (ic[0] + ic[1]) + ic[2];
  return pe * (((U[0] * J0 + U[1] * J1) + U[2] * J2) + U[3] * J3);
}

// the row on lane `lane` of the staged tile: the walk over the list, LDS and registers only; leaves D of every branch in the
// father's slot and R
GPH_SM_FN void gph_mu_row(const GphMuLds &s, const GphLayout &y, const GphMuShape &h, int lane, int root)
{
  const int n = y.n, N = y.N, TR = h.TR, nord = s.ord[0], slots = 4 * (n - 1) * TR;
  for (int k = 0; k < nord; k++) {
    const int v = s.ord[GPH_IX(1 + k, n)], l = s.nd[GPH_IX(v, N)].left, rr = s.nd[GPH_IX(v, N)].right;
    if ((unsigned)l >= (unsigned)N || (unsigned)rr >= (unsigned)N) continue;      /* (a damaged record must not reach past the arrays) */
    double O[4], il[4], ir[4], fl[4], fr[4], ol[4], orr[4];
    if (v == root) {                                /* its slot still holds its own conditionals */
      gph_mu_inside(s, n, TR, lane, v, O);
      s.R[GPH_IX(lane, TR)] = ((O[0] + O[1]) + O[2]) + O[3];
      for (int x = 0; x < 4; x++) O[x] = 1.0;
    } else {
      for (int x = 0; x < 4; x++) O[x] = s.park[GPH_IX((v - n) * 4 * TR + x * TR + lane, slots)];
    }
    gph_mu_inside(s, n, TR, lane, l, il);
    gph_mu_inside(s, n, TR, lane, rr, ir);
    const double pl = s.pe[GPH_IX(l, N)], ql = s.qe[GPH_IX(l, N)], pr = s.pe[GPH_IX(rr, N)], qr = s.qe[GPH_IX(rr, N)];
    gph_mu_factor(il, pl, ql, fl);
    gph_mu_factor(ir, pr, qr, fr);
    const double Dl = gph_mu_down(O, fr, il, pl, ql, ol), Dr = gph_mu_down(O, fl, ir, pr, qr, orr);
    if (l >= n && l != v)
      for (int x = 0; x < 4; x++) s.park[GPH_IX((l - n) * 4 * TR + x * TR + lane, slots)] = ol[x];
    if (rr >= n && rr != v)
      for (int x = 0; x < 4; x++) s.park[GPH_IX((rr - n) * 4 * TR + x * TR + lane, slots)] = orr[x];
    s.park[GPH_IX((v - n) * 4 * TR + lane, slots)] = Dl;
    s.park[GPH_IX((v - n) * 4 * TR + TR + lane, slots)] = Dr;
  }
}

// the open column of branch c closed: Dv = Dv + count d
GPH_SM_FN void gph_mu_close(double *car, int N, int c)
{
  const double DD = car[GPH_IX(MU_DD * N + c, MU_WORDS * N)], RR = car[GPH_IX(MU_RR * N + c, MU_WORDS * N)];
  const double d = RR == 0.0 ? 0.0 : DD / RR;
  car[GPH_IX(MU_DV * N + c, MU_WORDS * N)] = car[GPH_IX(MU_DV * N + c, MU_WORDS * N)] + car[GPH_IX(MU_CNT * N + c, MU_WORDS * N)] * d;
}

// branch c over the `rows` rows of the tile, in row order; the column state is read once and written once
GPH_SM_FN void gph_mu_columns_of(const GphMuLds &s, const GphMuShape &h, int n, int N, int c, int rows)
{
  const int f = gph_mu_father(s, n, N, c), TR = h.TR;
  if (f < 0) return;
  const double *D = s.park + (size_t)GPH_IX((f - n) * 4 * TR + (s.nd[GPH_IX(f, N)].left == c ? 0 : TR), 4 * (n - 1) * TR);
  double *car = s.car;
  double DD = car[GPH_IX(MU_DD * N + c, MU_WORDS * N)], RR = car[GPH_IX(MU_RR * N + c, MU_WORDS * N)], Dv = car[GPH_IX(MU_DV * N + c, MU_WORDS * N)];
  double count = car[GPH_IX(MU_CNT * N + c, MU_WORDS * N)], sites = car[GPH_IX(MU_SITES * N + c, MU_WORDS * N)];
  for (int r = 0; r < rows; r++) {
    if (s.ph[GPH_IX(r, TR)] != 0) {
      Dv = Dv + count * (RR == 0.0 ? 0.0 : DD / RR);        /* the open column closed */
      DD = 0.0; RR = 0.0;
      count = (double)s.cnt[GPH_IX(r, TR)];
      sites += count;                                       /* (integers below 2^53: exact) */
    }
    DD = DD + D[GPH_IX(r, TR)];
    RR = RR + s.R[GPH_IX(r, TR)];
  }
  car[GPH_IX(MU_DD * N + c, MU_WORDS * N)] = DD; car[GPH_IX(MU_RR * N + c, MU_WORDS * N)] = RR; car[GPH_IX(MU_DV * N + c, MU_WORDS * N)] = Dv;
  car[GPH_IX(MU_CNT * N + c, MU_WORDS * N)] = count; car[GPH_IX(MU_SITES * N + c, MU_WORDS * N)] = sites;
}

// M_c of branch c from its column sums (0 where there is no branch or u == 0)
GPH_SM_FN void gph_mu_expected(const GphMuLds &s, int n, int N, int c, double rate)
{
  double *car = s.car;
  double M = 0.0;
  const int f = gph_mu_father(s, n, N, c);
  const double pe = s.pe[GPH_IX(c, N)];
  if (f >= 0 && pe > 0.0) {
    gph_mu_close(car, N, c);
    const double len = rate * (s.nd[GPH_IX(f, N)].age - s.nd[GPH_IX(c, N)].age);
    const double a = -gph_quot(-4 * len, 3.0, 1.0 / 3.0), u = 1 - gph_exp(gph_quot(-4 * len, 3.0, 1.0 / 3.0)), qe = s.qe[GPH_IX(c, N)];
    const double Ediff = (a * qe) / u + 0.75 * a, Esame = ((0.75 * a) * u) / (1 + 3 * qe);
    const double Dv = car[GPH_IX(MU_DV * N + c, MU_WORDS * N)], sites = car[GPH_IX(MU_SITES * N + c, MU_WORDS * N)];
    M = Esame * (sites - Dv) + Ediff * Dv;
  }
  car[GPH_IX(MU_M * N + c, MU_WORDS * N)] = M;
}

// the population segments of the branch above v in time order: emit(p, dt) for each.  Every loop is bounded: nm + 1 events,
// K populations climbed before each
extern "C++" { template <class Emit> GPH_SM_FN void gph_mu_segments(const GphMuLds &s, const GphLayout &y, int nm, int v, Emit emit)
{
  const int n = y.n, N = y.N, K = y.K, B = y.B;
  const int16_t *living = s.migi + GPH_MAX_MIGS * MG_COUNT;
  const int f = gph_mu_father(s, n, N, v);
  if (f < 0 || !(s.pe[GPH_IX(v, N)] > 0.0)) return;
  const double top = s.nd[GPH_IX(f, N)].age;
  int cur = s.nd[GPH_IX(v, N)].npop;
  double t = s.nd[GPH_IX(v, N)].age;
  uint32_t used = 0;
  for (int step = 0; step <= nm; step++) {
    int pick = -1;                                  /* the next live migration on this branch: the youngest not taken, the first of equals */
    double b = top;
    for (int k = 0; k < nm; k++) {
      const int mg = living[GPH_IX(k, GPH_MAX_MIGS)];
      if ((used >> k) & 1u || (unsigned)mg >= (unsigned)GPH_MAX_MIGS) continue;
      if (s.migi[GPH_IX(mg * MG_COUNT + MG_BRANCH, GPH_MAX_MIGS * MG_COUNT)] != v) continue;
      const double ag = s.mage[GPH_IX(mg, GPH_MAX_MIGS)];
      if (pick < 0 || ag < b) { pick = k; b = ag; }
    }
    for (int guard = 0; guard < K; guard++) {
      if ((unsigned)cur >= (unsigned)K) break;
      const int F = s.mpf[GPH_IX(cur, K + B)];
      if ((unsigned)F >= (unsigned)K) break;
      const double tau = s.mpa[GPH_IX(F, K)];
      if (!(tau <= b)) break;
      emit(cur, tau - t);
      cur = F; t = tau;
    }
    emit(cur, b - t);
    t = b;
    if (pick < 0) break;
    used |= 1u << pick;
    const int band = s.migi[GPH_IX(living[GPH_IX(pick, GPH_MAX_MIGS)] * MG_COUNT + MG_BAND, GPH_MAX_MIGS * MG_COUNT)];
    cur = (unsigned)band < (unsigned)B ? s.mpf[GPH_IX(K + band, K + B)] : -1;
  }
} }

// branch v: its segments with their two terms into the lists (the first h.segcap of them; the count says how many there were)
GPH_SM_FN void gph_mu_list(const GphMuLds &s, const GphLayout &y, const GphMuShape &h, int nm, int v, double rate, double sites)
{
  const int N = y.N, cap = h.segcap;
  const int f = gph_mu_father(s, y.n, N, v);
  const double Mv = s.car[GPH_IX(MU_M * N + v, MU_WORDS * N)], tv = f >= 0 ? s.nd[GPH_IX(f, N)].age - s.nd[GPH_IX(v, N)].age : 0.0;
  int k = 0;
  gph_mu_segments(s, y, nm, v, [&](int p, double dt) {
    if (k < cap) {
      s.segp[GPH_IX(v * cap + k, N * cap)] = (int16_t)p;
      s.segm[GPH_IX(v * cap + k, N * cap)] = Mv * (dt / tv);
      s.segx[GPH_IX(v * cap + k, N * cap)] = (rate * dt) * sites;
    }
    k++;
  });
  s.segn[GPH_IX(v, N)] = (int16_t)k;
}

// population p: mut_p and exp_p of the locus, nodes in index order, segments in time order -- from the lists, and for a branch
// whose segments outgrew its list by walking them again
GPH_SM_FN void gph_mu_population(const GphMuLds &s, const GphLayout &y, const GphMuShape &h, int nm, int p, double rate, double sites, double &mut, double &ex)
{
  const int N = y.N, cap = h.segcap;
  mut = 0.0; ex = 0.0;
  for (int v = 0; v < N; v++) {
    const int k = cap > 0 ? s.segn[GPH_IX(v, N)] : cap + 1;
    if (k <= cap) {
      for (int i = 0; i < k; i++)
        if (s.segp[GPH_IX(v * cap + i, N * cap)] == p) { mut = mut + s.segm[GPH_IX(v * cap + i, N * cap)]; ex = ex + s.segx[GPH_IX(v * cap + i, N * cap)]; }
      continue;
    }
    const int f = gph_mu_father(s, y.n, N, v);
    const double Mv = s.car[GPH_IX(MU_M * N + v, MU_WORDS * N)], tv = f >= 0 ? s.nd[GPH_IX(f, N)].age - s.nd[GPH_IX(v, N)].age : 0.0;
    gph_mu_segments(s, y, nm, v, [&](int q, double dt) {
      if (q == p) { mut = mut + Mv * (dt / tv); ex = ex + (rate * dt) * sites; }
    });
  }
}

// workgroup w = block bx: the selected loci w chunk ... of the rank.  acc [nsel][C]; part [chunks][1 + C] (column 0 is the
// fold's iteration column)
GPH_FLAT(k_mutations, GPH_MU_THREADS, GphKargs KA, GphMuShape h, const char *pages, const char *condb, const uint64_t *cond_off, const char *seq,
         const uint64_t *seq_off, const int32_t *P2, const int32_t *sel_slot, int nsel, int L, double *acc, double *part)
{
  GPH_FLAT_BODY(GphNoLane);
  const GphLayout &y = KA.lay;
  const GphModel &model = KA.G->model;
  const int n = y.n, N = y.N, K = y.K, B = y.B, C = h.C, TR = h.TR;
  const int q0 = bx * h.chunk, live = nsel - q0 < h.chunk ? nsel - q0 : h.chunk;
  if (live <= 0) return;
  GphMuLds s;
  gph_mu_carve(lds, h, s);
  GPH_PHASE {
    for (int c = tid; c < C; c += bd) s.prow[GPH_IX(c, C)] = 0.0;
    /* the population tree as the chain state has it, once: the walks read it many times */
    for (int p = tid; p < K; p += bd) { s.mpa[GPH_IX(p, K)] = model.popAge[p]; s.mpf[GPH_IX(p, K + B)] = (int16_t)model.popFather[p]; }
    for (int b = tid; b < B; b += bd) s.mpf[GPH_IX(K + b, K + B)] = (int16_t)model.bandSrc[b];
  }
  for (int g = 0; g < live; g++) {
    const int q = q0 + g, j = GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
    const int P = P2[GPH_IX(2 * j, 2 * L)];
    const char *pg = pages + (size_t)j * y.page_bytes, *blk = seq + seq_off[GPH_IX(j, L + 1)];
    const double *cond = (const double *)(condb + cond_off[GPH_IX(j, L + 1)]);
    const int32_t *is = (const int32_t *)(pg + y.o_iscal);
    const double rate = ((const double *)(pg + y.o_fscal))[FS_MUTRATE];
    const int root = is[IS_ROOT];
    int nm = is[IS_NUM_MIGS];
    nm = nm < 0 ? 0 : nm > GPH_MAX_MIGS ? GPH_MAX_MIGS : nm;
    GPH_PHASE {
      for (int v = tid; v < N; v += bd) {
        gph_copy16(s.nd + GPH_IX(v, N), pg + y.o_nd + (size_t)v * 16);
        s.cb[GPH_IX(v, N)] = (int16_t)(((uint32_t)is[IS_CBIT0 + (v >> 5)] >> (v & 31)) & 1u);
      }
      for (int k = tid; k < MU_WORDS * N; k += bd) s.car[GPH_IX(k, MU_WORDS * N)] = 0.0;
      for (int k = tid; k < GPH_MAX_MIGS; k += bd) {
        s.mage[GPH_IX(k, GPH_MAX_MIGS)] = ((const double *)(pg + y.o_mig_age))[k];
        s.migi[GPH_IX(GPH_MAX_MIGS * MG_COUNT + k, GPH_MAX_MIGS * (MG_COUNT + 1))] = ((const int16_t *)(pg + y.o_living))[k];
      }
      for (int k = tid; k < GPH_MAX_MIGS * MG_COUNT; k += bd) s.migi[GPH_IX(k, GPH_MAX_MIGS * (MG_COUNT + 1))] = ((const int16_t *)(pg + y.o_mig_i))[k];
    }
    GPH_BARRIER;
    GPH_PHASE {
      for (int v = tid; v < N; v += bd) gph_mu_edge(s, n, N, v, rate);
      if (tid == bd - 1) gph_mu_order(s, n, N, root);      /* (the last lane: at 16 leaves it has no node of its own) */
    }
    GPH_BARRIER;
    for (int r0 = 0; r0 < P; r0 += TR) {
      const int rows = P - r0 < TR ? P - r0 : TR;
      GPH_PHASE {
        gph_mu_stage_tile(s, y, h, blk, cond, P, r0, rows, tid, bd);
      }
      GPH_BARRIER;
      GPH_PHASE {
        for (int lane = tid; lane < rows; lane += bd) gph_mu_row(s, y, h, lane, root);
      }
      GPH_BARRIER;
      GPH_PHASE {
        for (int c = tid; c < N; c += bd) gph_mu_columns_of(s, h, n, N, c, rows);
      }
      GPH_BARRIER;
    }
    GPH_PHASE {
      for (int c = tid; c < N; c += bd) gph_mu_expected(s, n, N, c, rate);
    }
    GPH_BARRIER;
    /* (the sites as any branch summed them: those of leaf 0, which always has a branch) */
    const double sites = s.car[GPH_IX(MU_SITES * N + 0, MU_WORDS * N)];
    if (h.segcap > 0) {
      GPH_PHASE {
        for (int v = tid; v < N; v += bd) gph_mu_list(s, y, h, nm, v, rate, sites);
      }
      GPH_BARRIER;
    }
    GPH_PHASE {
      for (int t = tid; t < K + n; t += bd) {
        double a, b;
        int ca, cb;
        if (t < K) {
          gph_mu_population(s, y, h, nm, t, rate, sites, a, b);
          ca = t; cb = K + t;
        } else {
          const int i = t - K, f = gph_mu_father(s, n, N, i);
          a = s.car[GPH_IX(MU_M * N + i, MU_WORDS * N)];
          b = f >= 0 ? (rate * (s.nd[GPH_IX(f, N)].age - s.nd[GPH_IX(i, N)].age)) * s.car[GPH_IX(MU_SITES * N + i, MU_WORDS * N)] : 0.0;
          ca = 2 * K + i; cb = 2 * K + n + i;
        }
        double *w = acc + (size_t)q * C;
        w[GPH_IX(ca, C)] = w[GPH_IX(ca, C)] + a;
        w[GPH_IX(cb, C)] = w[GPH_IX(cb, C)] + b;
        s.prow[GPH_IX(ca, C)] = s.prow[GPH_IX(ca, C)] + a;
        s.prow[GPH_IX(cb, C)] = s.prow[GPH_IX(cb, C)] + b;
      }
    }
    GPH_BARRIER;
  }
  GPH_PHASE {
    double *out = part + (size_t)bx * (1 + C);
    if (tid == 0) out[0] = 0.0;
    for (int c = tid; c < C; c += bd) out[1 + c] = s.prow[GPH_IX(c, C)];
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
