// gph_genetrees.h -- k_gene_trees: the sampled genealogies of selected loci, gathered on the device (include/gphocs_hip.h,
// gph_engine_gene_trees_*).
//
// What is gathered.  One RECORD describes one locus at one sample: the node records (age, father, left, right, npop of the
// N = 2n - 1 nodes), mig_age, the mig_i words with `living`, and the page scalars that hold the two log-likelihoods, the
// root and the number of live migrations -- what the LOCUS, N and M lines of a state dump print.  A record is the packed
// image (gph_sampler.h) of five 16-byte-aligned byte ranges of the page, verbatim: nd[0 .. N), mig_age, fscal ..
// iscal[IS_ROOT] (the two arrays lie next to each other in GphLds: one range), iscal[IS_NUM_MIGS] (the node sets between the
// two words grow with the leaf capacity and are left out) and mig_i .. living (neighbours too: one range).  The image holds
// five ranges, which is what GPH_PACK_RANGES allows; nothing changes for its other users.  A record has no header;
// gph_gt_shape gives its byte size and the offsets of the arrays inside it, and gph_gene_trees_decode (host) turns it into
// plain arrays: migrations in `living` order, IS_NUM_MIGS clamped as gph_an_num_migs clamps it.
//
// Layout.  A sample's ROW is [q][record bytes], q = 0 .. nsel - 1 over the selected loci of the rank in increasing locus
// index.  Slots are sorted by decreasing pattern count, so record q comes from slot sel_slot[q] (a table in HBM).
//
// Shape.  A gather, one 16-byte unit a lane, one 128-bit load and one 128-bit store each.  Workgroup w takes the G =
// max(1, 256 / units) consecutive records w G ... of the row (units = 16-byte units of a record: 50 at 16 leaves, G = 5 and
// 250 of 256 lanes at work); lane t copies unit t % units of its t / units-th record, so consecutive lanes write consecutive
// units of the row (the stores coalesce fully) and read consecutive units of a range (the loads coalesce within a range: at
// 16 leaves the node range alone is 496 of a record's 800 bytes).  A record of more than 256 units (above 118 leaves) takes
// its workgroup more than one trip.  All index arithmetic is 32-bit (a flat unit index over the whole row would need a
// 64-bit division a lane, which costs as much as the copy).  No LDS, no atomics; nothing grows with the band capacity.  16 N + 288 bytes a record (up to 16 more where a
// range straddles a boundary): 0.8 KB at 16 leaves, 2.6 KB at 72.
//
// The kernel has one text (the flat-kernel form, gph_sampler.h): the host-emulation build runs it lane by lane, phase by phase.
// It writes no page, draws no random number and touches no chain state.
#pragma once
#include "gph_sampler.h"

#undef GPH_FILE_ID
#define GPH_FILE_ID 8

#define GPH_GT_THREADS 256
#define GPH_GT_RANGES 5
static_assert(GPH_GT_RANGES <= GPH_PACK_RANGES, "a record is one packed image");

// record offsets of what a record holds (the C ABI hands them out in this order: gph_engine_gene_trees_shape)
enum { GT_O_NODES = 0, GT_O_ROOT, GT_O_NUM_MIGS, GT_O_DATALNL, GT_O_GENLNL, GT_O_MIG_AGE, GT_O_MIG_I, GT_O_LIVING, GT_O_COUNT };

struct GphGtShape {
  GphPackedImg img;
  int32_t off[GT_O_COUNT];
  int32_t units;              // 16-byte units of a record (img.bytes / 16)
  int32_t G;                  // records a workgroup
};

GPH_SM_HD void gph_gt_shape(const GphLayout &y, GphGtShape &h)
{
  const int lo[GPH_GT_RANGES] = {y.o_nd, y.o_mig_age, y.o_fscal, y.o_iscal + IS_NUM_MIGS * 4, y.o_mig_i};
  const int sz[GPH_GT_RANGES] = {y.N * 16, GPH_MAX_MIGS * 8, (y.o_iscal - y.o_fscal) + (IS_ROOT + 1) * 4, 4,
                                 (y.o_living - y.o_mig_i) + GPH_MAX_MIGS * 2};
  int a[GPH_GT_RANGES];
  gph_pack_ranges(y, lo, sz, GPH_GT_RANGES, h.img, a);
  h.off[GT_O_NODES] = a[0];
  h.off[GT_O_MIG_AGE] = a[1];
  h.off[GT_O_DATALNL] = a[2] + FS_DATALNL * 8;
  h.off[GT_O_GENLNL] = a[2] + FS_GENLNL * 8;
  h.off[GT_O_ROOT] = a[2] + (y.o_iscal - y.o_fscal) + IS_ROOT * 4;
  h.off[GT_O_NUM_MIGS] = a[3];
  h.off[GT_O_MIG_I] = a[4];
  h.off[GT_O_LIVING] = a[4] + (y.o_living - y.o_mig_i);
  h.units = h.img.bytes / 16;
  h.G = h.units < GPH_GT_THREADS ? GPH_GT_THREADS / h.units : 1;
}

// unit t of workgroup w (t < G units): where it is read in the pages and where it is written in the row (byte offsets);
// false: beyond the last record
GPH_SM_FN bool gph_gt_unit(const GphLayout &y, const GphGtShape &h, const int32_t *sel_slot, int nsel, int L, int w, int t, size_t &src, size_t &dst)
{
  const int g = t / h.units, o = (t - g * h.units) * 16, q = w * h.G + g;
  if (q >= nsel) return false;
  const int j = GPH_IX(sel_slot[GPH_IX(q, nsel)], L);
  src = (size_t)j * y.page_bytes + (size_t)GPH_IX(gph_pack_unit_src(h.img, GPH_IX(o, h.img.bytes)), y.page_bytes);
  dst = (size_t)q * h.img.bytes + (size_t)o;
  return true;
}

// workgroup w = block bx
GPH_FLAT(k_gene_trees, GPH_GT_THREADS, GphLayout y, GphGtShape h, const char *pages, const int32_t *sel_slot, int nsel, int L, char *row)
{
  GPH_FLAT_BODY(GphNoLane);
  GPH_PHASE {
    for (int t = tid; t < h.G * h.units; t += GPH_GT_THREADS) {
      size_t src, dst;
      if (gph_gt_unit(y, h, sel_slot, nsel, L, bx, t, src, dst)) gph_copy16(row + dst, pages + src);
    }
  }
}

#undef GPH_FILE_ID
#define GPH_FILE_ID 2
