/* oracle/ref_zero_heap.h -- TEST INFRASTRUCTURE ONLY, forced into the objects of the reference's patch.c by oracle/Makefile
 * (-include).  The reference reads heap cells it never wrote: createEvent (patch.c:1680-1700) leaves an event's node_id as
 * the slot held it, and a SAMPLES_START event (patch.c:2028-2032) never gets one, so the canonical state dump of the harness
 * would print whatever the allocator handed out -- zero in a small run, the bytes of a freed sequence buffer in a run with
 * 2000-bp loci.  With malloc as calloc the harness is a function of its inputs; no decision of the chain reads those cells. */
#ifndef GPH_REF_ZERO_HEAP_H
#define GPH_REF_ZERO_HEAP_H
#include <stdlib.h>
#define malloc(n) calloc(1, (n))
#endif
