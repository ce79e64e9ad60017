// partials_fused.hpp -- plan of the site-blocked whole-list kernels: planner and the 20-state list's classes, certificate
// bounds and walk (fused_plan.hip), kernels (partials_fused.hip, 4 states; partials_aa_fused.hip, 20); the 4-state
// list's record, index rule and gather descriptors, one definition each for the kernel, the encoder and the host
#ifndef PLLHIP_PARTIALS_FUSED_HPP_
#define PLLHIP_PARTIALS_FUSED_HPP_

#include <utility>
#include <vector>

#include "ctx.hpp"

constexpr int PLLHIP_FUSED_J = 2; // sub-steps (64 lanes x 16 B) per tile

// One LDS slot of a wave: a tile and its scaler counts -- `count_words` per sub-step: one per site (four at least),
// 32 with per-rate scalers.  (Slots per wave, the launch's LDS and the records' byte offsets all come from here.)
struct FusedSlotSize
{
  unsigned int count_words, tile_bytes, count_bytes;
  unsigned int bytes() const { return tile_bytes + count_bytes; }
};
inline FusedSlotSize pllhip_fused_slot_size(unsigned int rate_cats, bool rate_scalers)
{
  const unsigned int sps = 64 / (2 * rate_cats); // sites per sub-step
  const unsigned int cw = rate_scalers ? 32 : (sps < 4 ? 4 : sps);
  return {cw, PLLHIP_FUSED_J * 64u * 16u, PLLHIP_FUSED_J * cw * 4u};
}

// A GATHERED operand: a factor the list kernel takes from a small table by tip characters instead of computing it
// from a CLV -- a tip, or a deferred cherry (deferred.hip: a tip-tip parent that is not stored).
enum { FUSED_G_NONE = 0, FUSED_G_TIP = 1, FUSED_G_PAIR = 2, FUSED_G_CHERRY_NEW = 3, FUSED_G_CHERRY_KEPT = 4 };
struct FusedOperand
{
  int type;                         // FUSED_G_*: TIP the tip's factor; PAIR the finished tip-tip parent (kind 2);
                                    // CHERRY_NEW a cherry deferred by this list, CHERRY_KEPT by an earlier call
  const unsigned char * row1;       // tip rows the table is indexed by: (row1 << 4) | row2; row2 nullptr: code 0
  const unsigned char * row2;
  const double * mat;               // the reader's P-matrix on this edge
  const double * c_lmat, * c_rmat;  // CHERRY_NEW: the cherry's own two matrices (its T is built from them on the spot)
  const double * kept;              // CHERRY_KEPT: its kept table T
  const unsigned char * row;        // the ONE row the kernel reads the table index from (pllhip_fused_gather_row): the
                                    // cached pair row of (row1, row2) -- set by the launch, pair_rows.hip --, else the tip row
};
// A side of an op may also be the PRODUCT of two gathered factors (prod[side] != 0): a gathered-gathered parent with one
// reader that is not walked at all but formed by that reader (pllhip_fused_fold).  g[side] and g2[side] are then its
// two factors; prod[side] is a bit set: 1 a product, | 2 the folded op has a scale buffer (its scaling test can fire),
// | 4 the reader passes its scale buffer on that side (it inherits the product's scale bit), | 8 the two factors are
// QUADS -- the folded op is itself a reader of two folded products, both read as quads, whose parent stays unstored
// (pllhip_fused_quad_fold_walk; the factors are then in FusedOp::q, filled from the plan before); pkeep[side]: where the
// two factor tables are kept (the pool: deferred.hip).
struct FusedExtra
{
  FusedOperand g[2];
  FusedOperand g2[2];
  int prod[2];
  double * pkeep[2][2];
};

// What the planner decides for one op (host side; the device gets FusedRec below).
struct FusedOp
{
  double * parent;
  const double * left_hbm;         // inner child 1 when it is copied into lslot from HBM (reload), else nullptr
  const double * right_hbm;        // the same for the inner child of "right"
  const unsigned char * ltip;      // tip child (tip-inner), tip child 1 (tip-tip), else nullptr
  const unsigned char * rtip;      // tip child 2 (tip-tip), else nullptr
  const double * lmat;
  const double * rmat;
  unsigned int * pscaler;          // nullptr: no scaling
  const unsigned int * lsc_hbm;    // counts copied into the slot together with left_hbm / right_hbm, else nullptr
  const unsigned int * rsc_hbm;
  int lslot, rslot, pslot;         // LDS slots of the two inner children / the parent; -1 = none
  int lsc_slot, rsc_slot;          // LDS slots the inherited counts are taken from; -1 = none
  int kind;                        // 0 inner-inner, 1 gathered-inner (tip or deferred cherry), 2 tip-tip, 3 gathered-gathered
  int list_pos;                    // position of the op in the caller's list (the plan is re-ordered)
  int dma_flags;                   // bit 0 / 1: left_hbm / right_hbm is copied into lslot / rslot by LDS-DMA
                                   // at the top of the op before this one
  const double * pair_tab;         // tip operands: [256 code pairs][rate][state] table, else nullptr
  FusedOperand g[2];               // gathered operands over deferred cherries (type 0: the op's kind says it all)
  int unstored;                    // kind 3: the parent is not stored (pllhip_fused_unstored) -- its CLV stores go to the sink
  double * keep[2];                // ... and its two factor tables are also written here (the pool: deferred.hip)
  // folded pair products (pllhip_fused_fold): side s is the product of the gathered factors g[s] and g2[s].  To the
  // planner the op is then gathered-inner (kind 1, the product "left") or gathered-gathered (kind 3); the kernel runs
  // it as an inner-inner op whose operand on that side is formed from registers instead of read from a slot.
  FusedOperand g2[2];
  int prod[2];                     // 0 no product; else bits: 1 a product, 2 its op has a scale buffer, 4 the reader inherits its count,
                                   // 8 a folded QUAD product: its two factors are the quads q[s][0], q[s][1]
  double * pkeep[2][2];            // the pool's places of the two factor tables of side s
  // a folded quad product on side s (prod[s] & 8): quad t of it is what side t of the folded op was in the plan before
  // -- a folded pair product over two cherries, a and b, read with the folded op's matrix on that side --, the places
  // of a's and b's factor tables in the pool; qkeep[s][t]: where the quad's table is kept (the pool of quad tables)
  struct Quad
  {
    FusedOperand a, b;
    const double * mat;
    double * pkeep[2];
  } q[2][2];
  double * qkeep[2][2];
};

// The plan as the kernel reads it, through the scalar data cache: ONE 64-byte record per op (one
// scalar load, one cache line; the gather descriptors of FusedPlanRec below lie behind it, a second
// load issued with it), holding everything the wave does WHILE that op runs, ready
// to use -- absolute addresses and LDS byte offsets, no indices to multiply out:
//   - what it requests for the op two ahead (P-matrix offsets),
//   - the pair table it gathers from for the op one ahead and where that op's tip characters are
//     (which lanes of the wave's character registers), what that op reloads and which of its
//     matrices must be staged,
//   - the op itself: parent, scale buffer, LDS places of operands, parent and counts.
// Round 2 first had 32-byte records of 16-bit indices, decoded by the kernel; the counters say
// a wave-op then cost 124 scalar + 124 vector instructions of which 30 were arithmetic, and that
// the wave, not HBM, was the limit (tools/pmc_instmix.sh) -- so the
// host now does the decoding once per list.  The records hold addresses: they are rebuilt when an
// arena moves (layout_epoch).  (The gathers added since brought a packed word back, chars .. chars4:
// the kernel no longer reads it but for CH_LOAD and its batch -- FusedGatherDesc holds the same,
// finished; the words are still written, for the host's tests and the batch switch.)
struct FusedRec
{
  unsigned int chars;                    // tip characters of op + 1, PLLHIP_FUSED_CH_* below
  unsigned int chars2;                   // ... of its SECOND gather (kind 3, a product), same layout (no CH_LOAD, no batch)
  unsigned int chars3, chars4;           // ... of a third and fourth one (a reader of folded products: up to four factors)
                                         // (the tables of one op follow each other: gather k reads at gather_off + k tables)
  unsigned int req_lmat, req_rmat;       // byte offsets of its P-matrices in the matrix arena
  unsigned int gather_off;               // byte offset of the pair table of op + 1 (read only if chars has CH_LTIP)
  unsigned int flags;                    // PLLHIP_FUSED_* below
  unsigned long long parent;             // CLV the op writes
  unsigned long long pscaler;            // its scale buffer (0: none)
  unsigned short lslot_b, rslot_b;       // LDS byte offsets (within the wave's slots) of the operands,
  unsigned short pslot_b, src;           //   of the parent; FusedSrc number of what op + 1 reloads
  unsigned short lcnt_b, rcnt_b;         // LDS byte offsets (within the wave's counts) the inherited
  unsigned short pcnt_b, list_pos;       //   counts are read from / the parent's are kept at
};
static_assert(sizeof(FusedRec) == 64, "sixteen words per op");
#define PLLHIP_FUSED_KIND_MASK 3u      /* 0 inner-inner, 1 gathered-inner, 2 tip-tip, 3 gathered-gathered */
#define PLLHIP_FUSED_HAS_PSLOT 4u      /* the parent is kept in a slot */
#define PLLHIP_FUSED_SCALING 8u        /* the op has a scale buffer */
#define PLLHIP_FUSED_LCNT 16u          /* counts are inherited from the left / right operand's slot */
#define PLLHIP_FUSED_RCNT 32u
#define PLLHIP_FUSED_STAGE_SHIFT 6     /* two bits: matrices op + 1 needs (2 both, 1 right only, 0 none) */
#define PLLHIP_FUSED_RELOAD_NEXT 256u  /* op + 1 reloads operands: FusedSrc number `src` */
#define PLLHIP_FUSED_UNSTORED 512u     /* the parent's CLV stores go to the wave's sink (a pair product: deferred.hip) */
#define PLLHIP_FUSED_LPROD 1024u       /* the left / right operand is the product of two gathered factors (sets 1, 2 / */
#define PLLHIP_FUSED_RPROD 2048u       /* 3, 4), formed at the top of the op instead of read from a slot               */
#define PLLHIP_FUSED_LPSCALE 4096u     /* ... and the folded op has a scale buffer: its scaling test runs              */
#define PLLHIP_FUSED_RPSCALE 8192u
#define PLLHIP_FUSED_KIND_EDGE 4        /* FusedOp::kind of the edge pseudo-op (never in a record's kind bits) */
#define PLLHIP_FUSED_MAX_OPS 60000u    /* longer lists run per level */
// FusedRec::chars -- a wave holds the characters of up to 1024 / (tile sites) tip rows at its tile, 16 bytes per
// lane, fetched with ONE load per tile (rows in the order the list uses them; lists with more tip operands fetch
// the next batch of rows when they get there):
#define PLLHIP_FUSED_CH_LPOS(x) ((x) & 0xffu)         /* first lane of the left tip's row (op + 1) */
#define PLLHIP_FUSED_CH_RPOS(x) (((x) >> 8) & 0xffu)  /* ... of the right tip's */
#define PLLHIP_FUSED_CH_LTIP (1u << 16)                /* op + 1 has a left / right tip */
#define PLLHIP_FUSED_CH_RTIP (1u << 17)
#define PLLHIP_FUSED_CH_LOAD (1u << 18)                /* op + 2's rows are in another batch: fetch batch (x >> 24) */
// A record's gathers name ONE row each (pair rows: pair_rows.hip): CH_LPOS is its first lane, CH_LTIP says that the
// factor is gathered at all, and
#define PLLHIP_FUSED_CH_SHIFT4 (1u << 19)              /* the row is a single tip's and the table's FIRST character: (code & 15) << 4 */
#define PLLHIP_FUSED_CH_NIBBLE (1u << 20)              /* the row is a single tip's: only the low nibble of a byte counts */
// The ONE rule for what a gathered factor with a first and / or a second tip row names (the encoder and
// pllhip_fused_plan_dry_rows): one row of a batch -- bit 0 of its pair of bits for pllhip_fused_char_batches8 --, and
// the bits of its chars word: none for a cherry's pair row (shift 0, every bit of a byte counts), the nibble mask and
// shift 4 for a single tip that is the table's first character, the mask and shift 0 for one that is its second.
inline unsigned int pllhip_fused_gather_rows(bool first, bool second) { return first || second ? 1u : 0u; }
inline unsigned int pllhip_fused_gather_bits(bool first, bool second)
{
  return first && second ? 0u : first ? (PLLHIP_FUSED_CH_SHIFT4 | PLLHIP_FUSED_CH_NIBBLE) : second ? PLLHIP_FUSED_CH_NIBBLE : 0u;
}

// ---- Pair rows.  Byte n of the pair row of the ordered tip pair (a, b) is the pair-table index of site n, joined
// from the two tip rows' characters.  ONE definition for the kernel that builds the rows
// (pair_rows.hip), the list kernel's tests and the host (tests/test_host_pair_rows.py).
__host__ __device__ constexpr unsigned char pllhip_pair_row_byte(unsigned char a, unsigned char b)
{
  return (unsigned char)(((a & 15u) << 4) | (b & 15u));
}
// ... four sites at a time, as the builder forms them (no byte carries into its neighbour)
__host__ __device__ constexpr unsigned int pllhip_pair_row_word(unsigned int a4, unsigned int b4)
{
  return ((a4 & 0x0f0f0f0fu) << 4) | (b4 & 0x0f0f0f0fu);
}

// ---- What k_dna_fused does on the scalar side: integer code on wave masks, no lane values.
// Plain C++, so the host runs the very functions (pllhip_fused_group_mask_dry, pllhip_fused_entry_bit_dry;
// tests/test_host_scalar_masks.py).

// The scaling rule's "all entries of the site (of the rate) are below the threshold" as mask arithmetic.  `below`: bit
// l set = both entries of lane l are below it (the two compares' own 64-bit results, and-ed).  Returns the mask in which
// all GW lanes of a group are set exactly where all GW of them were set in `below`: the and of the mask with itself
// shifted by 1, 2, 4, 8 as far as GW needs has, at a group's base lane, the and over the group; those bits alone are
// kept and spread over their groups (groups do not overlap: the multiplication by 2^GW - 1 carries nothing).
template <unsigned int GW>
__host__ __device__ constexpr unsigned long long pllhip_fused_group_base()
{
  static_assert(GW == 2 || GW == 4 || GW == 8 || GW == 16, "a site's lanes, or a rate's");
  return GW == 2 ? 0x5555555555555555ull : GW == 4 ? 0x1111111111111111ull : GW == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
}
template <unsigned int GW>
__host__ __device__ constexpr unsigned long long pllhip_fused_group_mask(unsigned long long below)
{
  unsigned long long m = below;
  m &= m >> 1;
  if (GW >= 4) m &= m >> 2;
  if (GW >= 8) m &= m >> 4;
  if (GW >= 16) m &= m >> 8;
  m &= pllhip_fused_group_base<GW>();
  return (m << GW) - m;
}
// The count bits of a tile's entries out of its sub-steps' group masks.  Entry t of the tile (lane t's: t < J * 64 / GW)
// is group t % EPS of sub-step t / EPS (EPS = 64 / GW groups per sub-step).  The sub-steps' base bits are laid side by
// side in ONE mask -- sub-step j's in bit j of each group, J <= GW -- so that a lane finds its entry's bit with one shift
// by a number that never changes, (t % EPS) * GW + t / EPS, whichever sub-step holds it.
template <unsigned int GW, unsigned int J>
__host__ __device__ constexpr unsigned long long pllhip_fused_entry_bits(const unsigned long long (&groups)[J])
{
  static_assert(J <= GW, "a group has a bit for every sub-step");
  unsigned long long bits = 0;
  for (unsigned int j = 0; j < J; ++j) bits |= (groups[j] & pllhip_fused_group_base<GW>()) << j;
  return bits;
}
template <unsigned int GW>
__host__ __device__ constexpr unsigned int pllhip_fused_entry_shift(unsigned int t)
{
  return (t % (64u / GW)) * GW + t / (64u / GW);
}

// ---- Quad rows (quad_rows.hip).  A QUAD is a folded pair product whose two factors are both cherries: its value at a
// site depends on the characters of four tips only, i.e. on the two pair-row bytes (pa, pb) of the site.  The distinct
// patterns (pa << 8) | pb of an alignment are numbered in ascending order -- the CLASSES -- and a quad row holds each
// site's class as a 16-bit number; the reader of the product gathers P . (Fa[pa] . Fb[pb]) from a per-call table of one
// entry per class instead of forming it.  ONE definition for the builder, the list kernel's index rule (below) and the host tests.
#define PLLHIP_QUAD_MAX_CLASSES 1024u
#define PLLHIP_FUSED_CH_WIDE (1u << 21)                /* the gather names a quad row: 16 bits per site, two lane positions per
                                                          row granule; in chars2 .. chars4, bits 24-31: tables the gathers before
                                                          it take beyond one each */
__host__ __device__ constexpr unsigned int pllhip_quad_pattern(unsigned char pa, unsigned char pb)
{
  return ((unsigned int)pa << 8) | pb;
}
// (a character code 0 -- no state at all -- makes the factor 0)
__host__ __device__ constexpr bool pllhip_quad_pattern_has_zero(unsigned int pattern)
{
  return !(pattern & 0xf000u) || !(pattern & 0x0f00u) || !(pattern & 0x00f0u) || !(pattern & 0x000fu);
}
// Where site n's 16 bits lie in a quad row of two planes of `stride` bytes each.  A wave fetches its tile's characters
// as 16-byte granules at row + first site of the tile, whatever the row (partials_fused.hip), so a quad row is laid out
// to be fetched the same way: granule g of plane 0 holds sites 16 g ... 16 g + 7, granule g of plane 1 sites 16 g + 8 ...
// 16 g + 15 -- the 32 bytes of sixteen sites are two lane positions of the character batch.
__host__ __device__ constexpr size_t pllhip_quad_row_offset(size_t n, size_t stride)
{
  return ((n >> 3) & 1u) * stride + (n >> 4) * 16u + (n & 7u) * 2u;
}
// Site n's class as read from a quad row in memory (deferred.hip: k_quad_product_materialise, and the host tests):
// the 16 bits at pllhip_quad_row_offset (an even offset: the builder stores whole granules of unsigned short).
__host__ __device__ inline unsigned int pllhip_quad_row_class(const unsigned char * row, size_t n, size_t stride)
{
  return *reinterpret_cast<const unsigned short *>(row + pllhip_quad_row_offset(n, stride));
}

// ---- The index rule.  A wave keeps its tile's character batch in LDS: PLLHIP_FUSED_BATCH_BYTES, lane position p's 16
// bytes at byte 16 p, as the one load of a tile fetched them -- so a byte row's TS bytes lie in a piece from 16 pos on,
// a quad row's two planes as two pieces, the second (lanes per row) x 16 bytes behind the first.  What lane `lane` reads
// of that block for sub-step j of the gather a record's character word `ch` describes, and the table index it forms of
// it: ONE definition for gather_factor() of k_dna_fused (through the gather descriptor below, which is what the kernel
// reads), the host (pllhip_fused_index_dry, tests/test_host_gather_index.py; pllhip_fused_gather_desc_dry) and the older
// dry entry points (pllhip_fused_row_index_dry, pllhip_fused_pair_index_dry, pllhip_fused_quad_pick_dry).
// Both forms read the ALIGNED 16 bits that hold the lane's entry -- a quad row's class whole, a byte row's byte as one
// half of them (`drop`: 0 or 8 bits below it) --, so that the kernel has one read instruction and no branch between the
// forms: they differ in numbers only.  The offset is the row's wave-uniform 16 pos plus a number of the lane's that
// never changes; the second sub-step's is the first's plus a constant.
#define PLLHIP_FUSED_BATCH_BYTES 1024u
struct FusedIndexRead
{
  unsigned int offset;            // byte offset into the wave's batch block (even)
  unsigned int width;             // bytes the lane reads there (2)
  unsigned int drop, mask, shift; // index = ((what was read >> drop) & mask) << shift: the entry's field, put in its place
  __host__ __device__ constexpr unsigned int field(unsigned int raw) const { return (raw >> drop) & mask; }
  __host__ __device__ constexpr unsigned int index(unsigned int raw) const { return field(raw) << shift; }
};

// ---- Gather descriptors.  Everything the rule above makes of a record's character word is a constant of the LIST -- the
// same for every tile and every wave --, so the encoder works it out once and the kernel reads FINISHED numbers: one
// descriptor per gathered factor of an op, up to four, behind the op's FusedRec (FusedPlanRec below).  The kernel tests
// no flag of the character word and derives nothing from it; what is left to a lane is one constant of its own
// (pllhip_fused_lane_pick) and the descriptor's numbers as operands.
//   table_off    the factor's table, in bytes from FusedBases::pairtab: gather_off + (k + displaced units) tables
//   form         PLLHIP_FUSED_GD_*: the other numbers, each where the instruction that takes it finds it -- the vector
//                unit's bit-field extract and its shifts read the low five bits of their operand only, so a number at
//                bit 0 IS an operand, and one at bit 8 or 16 after one scalar shift of the word
// Two words, not four: sixteen words of descriptors live across the op boundary did not fit the scalar registers of the
// instance with an edge epilogue and per-site scaling (reads of spilled registers inside the op loop); eight do.
struct FusedGatherDesc
{
  unsigned int table_off;
  unsigned int form;
};
static_assert(sizeof(FusedGatherDesc) == 8, "two words per factor");
// FusedGatherDesc::form
//   bits 0-4   PICK: 8 the byte forms, 16 the wide form.  Three uses: the bit at which the form's read offset begins in
//              the lane's constant; and-ed with that constant, the lane's `drop` (bit 3: a byte form's odd sites drop 8
//              bits); and, at 8 sites per sub-step, the bytes between the two sub-steps' reads -- at 4, 16 and 32 sites the
//              two forms have the same stride, the sites per sub-step (pllhip_fused_gather_stride)
//   bit 7      the factor is gathered at all
//   bits 8-12  BITS: the field's width, 16, 8 or 4 (FusedIndexRead::mask is (1 << BITS) - 1)
//   bits 16-19 SHIFT: the rule's shift plus the instance's log2 of a table entry's bytes, in one (12 at most)
//   bits 20-31 LDS: the byte offset of the row in the wave's batch block, 16 CH_LPOS (bits 20-23 are 0: what reads
//              SHIFT as five bits reads SHIFT)
#define PLLHIP_FUSED_GD_PICK(f) ((f) & 31u)
#define PLLHIP_FUSED_GD_PRESENT (1u << 7)
#define PLLHIP_FUSED_GD_BITS(f) (((f) >> 8) & 31u)
#define PLLHIP_FUSED_GD_SHIFT(f) (((f) >> 16) & 31u)
#define PLLHIP_FUSED_GD_LDS(f) ((f) >> 20)
#define PLLHIP_FUSED_GD_PICK_BYTE 8u
#define PLLHIP_FUSED_GD_PICK_WIDE 16u
// The record and its descriptors as the device reads them: 128 bytes per op, the descriptors a scalar load of their own
// behind the record (the rest is padding: a record and its descriptors never straddle more cache lines than they fill).
struct FusedPlanRec
{
  FusedRec rec;
  FusedGatherDesc gd[4];
  unsigned int pad[8];
};
static_assert(sizeof(FusedPlanRec) == 128, "a record, four descriptors, padding");
// (the vector unit's v_bfe_u32: offset and width are the low five bits of their operands)
__host__ __device__ constexpr unsigned int pllhip_fused_bfe(unsigned int x, unsigned int offset, unsigned int width)
{
  return (width & 31u) == 0u ? 0u : (x >> (offset & 31u)) & ((1u << (width & 31u)) - 1u);
}
// The bytes between the reads of sub-step 0 and sub-step 1: site SPS + s lies that far behind site s in both forms, and
// in the same half of its 16 bits (SPS is even).
template <unsigned int SPS>
__host__ __device__ constexpr unsigned int pllhip_fused_gather_stride(unsigned int form)
{
  static_assert(SPS == 4 || SPS == 8 || SPS == 16 || SPS == 32, "sites per sub-step");
  constexpr unsigned int TS = PLLHIP_FUSED_J * SPS, LPR = TS >= 16 ? TS / 16 : 1;
  static_assert(SPS == 4 || pllhip_quad_row_offset(SPS, LPR * 16u) == (SPS == 8 ? PLLHIP_FUSED_GD_PICK_WIDE : SPS), "the wide form's stride");
  static_assert(SPS != 8 || SPS == PLLHIP_FUSED_GD_PICK_BYTE, "the byte forms' stride at 8 sites");
  return SPS == 8 ? PLLHIP_FUSED_GD_PICK(form) : SPS;
}
// The descriptor of gather `k` of an op, from what the encoder has: the gather's character word, the op's gather_off
// and the instance's numbers -- log2 of an entry's bytes, bytes of a table.  (A gather behind the first finds its table
// behind all the tables of those before it: k of them, and what a wide gather's word counts in its top byte -- the
// first word's top byte is the batch of CH_LOAD.)  The 64-bit offset is for the encoder's check.
__host__ __device__ constexpr unsigned long long pllhip_fused_gather_table_off(unsigned int ch, unsigned int k, unsigned int gather_off,
                                                                                unsigned int table_bytes)
{
  const unsigned int units = (k >= 1u && (ch & PLLHIP_FUSED_CH_WIDE)) ? ch >> 24 : 0u;
  return (unsigned long long)gather_off + (unsigned long long)(k + units) * table_bytes;
}
__host__ __device__ constexpr FusedGatherDesc pllhip_fused_gather_desc(unsigned int ch, unsigned int k, unsigned int gather_off,
                                                                       unsigned int entry_shift, unsigned int table_bytes)
{
  const bool wide = (ch & PLLHIP_FUSED_CH_WIDE) != 0u;
  const unsigned int bits = wide ? 16u : (ch & PLLHIP_FUSED_CH_NIBBLE) ? 4u : 8u;
  const unsigned int shift = (!wide && (ch & PLLHIP_FUSED_CH_SHIFT4) ? 4u : 0u) + entry_shift;
  return {(unsigned int)pllhip_fused_gather_table_off(ch, k, gather_off, table_bytes),
          (wide ? PLLHIP_FUSED_GD_PICK_WIDE : PLLHIP_FUSED_GD_PICK_BYTE) | ((ch & PLLHIP_FUSED_CH_LTIP) ? PLLHIP_FUSED_GD_PRESENT : 0u) |
              bits << 8 | shift << 16 | (PLLHIP_FUSED_CH_LPOS(ch) * 16u) << 20};
}
// The lane's constant: its site of sub-step 0 as each form reads it -- the byte forms' offset (the aligned 16 bits that
// hold the site's byte) from bit 8, the wide form's (pllhip_quad_row_offset) from bit 16 -- and in bit 3 the 8 bits a
// byte form drops below an odd site's byte.
template <unsigned int SPS>
__host__ __device__ constexpr unsigned int pllhip_fused_lane_pick(unsigned int lane)
{
  static_assert(SPS == 4 || SPS == 8 || SPS == 16 || SPS == 32, "sites per sub-step");
  constexpr unsigned int TS = PLLHIP_FUSED_J * SPS, LPR = TS >= 16 ? TS / 16 : 1;
  const unsigned int site = lane / (64u / SPS);
  return (site & 1u) * 8u | (site & ~1u) << PLLHIP_FUSED_GD_PICK_BYTE |
         (unsigned int)pllhip_quad_row_offset(site, LPR * 16u) << PLLHIP_FUSED_GD_PICK_WIDE;
}
// What lane `lane` reads for sub-step j of the gather a descriptor describes, and what becomes of it: the statements of
// index_reads() and gather() of k_dna_fused, written out (shift: the descriptor's, the entry's bytes included).
template <unsigned int SPS>
__host__ __device__ constexpr FusedIndexRead pllhip_fused_index_of_desc(const FusedGatherDesc & d, unsigned int j, unsigned int lane)
{
  const unsigned int pick = pllhip_fused_lane_pick<SPS>(lane);
  return {PLLHIP_FUSED_GD_LDS(d.form) + pllhip_fused_bfe(pick, d.form, 8u) + j * pllhip_fused_gather_stride<SPS>(d.form), 2u,
          (d.form & pick) & 31u, (1u << PLLHIP_FUSED_GD_BITS(d.form)) - 1u, PLLHIP_FUSED_GD_SHIFT(d.form)};
}
// The rule of a character word: its descriptor's (no table, no entry size: the index as a number of entries).
template <unsigned int SPS>
__host__ __device__ constexpr FusedIndexRead pllhip_fused_index(unsigned int ch, unsigned int j, unsigned int lane)
{
  return pllhip_fused_index_of_desc<SPS>(pllhip_fused_gather_desc(ch, 0u, 0u, 0u, 0u), j, lane);
}
// ... applied to an image of the block (the host's dry entry points; the kernel reads its LDS)
template <unsigned int SPS>
inline unsigned int pllhip_fused_index_of_image(const unsigned char * image, unsigned int ch, unsigned int j, unsigned int lane)
{
  const FusedIndexRead rd = pllhip_fused_index<SPS>(ch, j, lane);
  unsigned int raw = 0;
  for (unsigned int b = 0; b < rd.width; ++b) raw |= (unsigned int)image[rd.offset + b] << (8u * b);
  return rd.index(raw);
}

// The ONE rule for whether a folded product is read as a quad (pllhip_launch_fused and pllhip_fused_quad_rule_dry).
// 0: taken; else why not.  n: the classes of its quad row (0: not counted -- beyond the cap); `scales`: the folded op
// has a scale buffer, and then `bound`, a lower bound on every entry of the table that needs no device (<= 0: none),
// must prove that the scaling rule cannot fire for any class: a gathered operand inherits no count.
enum
{
  FUSED_QUAD_TAKEN = 0,
  FUSED_QUAD_NOT_CHERRIES = 1, // a factor is a single tip
  FUSED_QUAD_INSTANCE = 2,     // quad rows are off, or the instance does not defer and fold
  FUSED_QUAD_CAP = 3,          // more than PLLHIP_QUAD_MAX_CLASSES classes
  FUSED_QUAD_RATIO = 4,        // fewer than min_sites_per_class sites per class
  FUSED_QUAD_BOUND = 5,        // the product might scale
  FUSED_QUAD_MIXED = 6         // the reader's other side is a folded product that is no quad
};
#define PLLHIP_QUAD_BOUND_MIN 0x1p-200
inline int pllhip_fused_quad_rule(bool cherries, bool instance, unsigned int n, unsigned int sites,
                                  unsigned int min_sites_per_class, bool scales, double bound)
{
  if (!instance) return FUSED_QUAD_INSTANCE;
  if (!cherries) return FUSED_QUAD_NOT_CHERRIES;
  if (n == 0 || n > PLLHIP_QUAD_MAX_CLASSES) return FUSED_QUAD_CAP;
  if ((unsigned long long)n * min_sites_per_class > sites) return FUSED_QUAD_RATIO;
  if (scales && !(bound >= PLLHIP_QUAD_BOUND_MIN)) return FUSED_QUAD_BOUND;
  return FUSED_QUAD_TAKEN;
}
// The rule over the folded products of a list (the live path's fused_pick_quads and pllhip_fused_plan_dry_quads): one
// candidate per product side of a walked op.  A reader of two products runs with both as quads or with neither -- the
// mixed reader is not built --, so a quad whose partner is none is refused as FUSED_QUAD_MIXED.  Returns the quads taken.
struct FusedQuadCand
{
  unsigned int seg, pos;   // the reader: its segment and position in the walk
  int side;                // 0: its left operand, 1: its right
  bool both;               // the reader's other operand is a folded product too
  bool cherries;           // both factors are cherries
  unsigned int n;          // classes of the quad row (0: not counted)
  bool scales;             // the folded op has a scale buffer
  double bound;            // lower bound of the table's entries the host can prove (<= 0: none)
  int reason;              // out: FUSED_QUAD_*
};
inline unsigned int pllhip_fused_quad_decide(FusedQuadCand * cands, size_t count, bool instance, unsigned int sites,
                                             unsigned int min_sites_per_class)
{
  for (size_t i = 0; i < count; ++i)
    cands[i].reason = pllhip_fused_quad_rule(cands[i].cherries, instance, cands[i].n, sites, min_sites_per_class, cands[i].scales, cands[i].bound);
  unsigned int taken = 0;
  for (size_t i = 0; i < count; ++i)
  {
    if (cands[i].reason != FUSED_QUAD_TAKEN || !cands[i].both) continue;
    bool partner = false;
    for (size_t k = 0; k < count; ++k)
      if (k != i && cands[k].seg == cands[i].seg && cands[k].pos == cands[i].pos && cands[k].side != cands[i].side)
        partner = cands[k].reason == FUSED_QUAD_TAKEN || cands[k].reason == -1;
    if (!partner) cands[i].reason = -1; // (marked: its partner still sees it as taken)
  }
  for (size_t i = 0; i < count; ++i)
  {
    if (cands[i].reason == -1) cands[i].reason = FUSED_QUAD_MIXED;
    taken += cands[i].reason == FUSED_QUAD_TAKEN;
  }
  return taken;
}

// sources and LDS destinations of the operands an op reloads (few ops have any: kept out of the records)
struct FusedSrc
{
  const double * left_hbm;
  const double * right_hbm;
  const unsigned int * lsc_hbm;
  const unsigned int * rsc_hbm;
  unsigned long long where; // lslot_b | rslot_b << 16 | lcnt_b << 32 | rcnt_b << 48
  unsigned long long pad;
};

// one pair table to build (k_dna_pair_tables)
// kind 0: [c1][0] = masksum4(lmat row, c1), a tip's factor; 1: [c1][c2] = masksum4(lmat) * masksum4(rmat), a tip-tip
// parent (tab in d_pairtab: a kept tip-tip op; in the pool: a deferred cherry's kept table T); 2: the READER's factor
// over a cherry, F[c1][c2][rate][s] = dot4(pmat[rate][s], T[c1][c2][rate][.]), T formed on the spot from lmat / rmat;
// 3: the same from the kept table `kept`
struct FusedPairJob
{
  const double * lmat;
  const double * rmat;
  double * tab;
  unsigned long long kind;
  const double * pmat;
  const double * kept;
  double * copy;                   // not nullptr: every entry is written here as well (an unstored pair product's factor)
  unsigned long long pad;
};

unsigned int pllhip_fused_char_batches(const unsigned int * tips, unsigned int count, unsigned int lpr,
                                       unsigned int * chars_out, unsigned int * batch_out);
// the same for ops with up to eight rows, the ONE batching rule (bits 2 k / 2 k + 1 of tips[pos]: the rows of gather k,
// into chars_out[k]; null outputs from the first unused)
unsigned int pllhip_fused_char_batches8(const unsigned int * tips, unsigned int count, unsigned int lpr,
                                        unsigned int * const chars_out[4], unsigned int * batch_out);

// Round 5: SEGMENTS.  Ops that share no buffer any of them writes are independent lists -- the two sides of the root
// edge of a full traversal, above all -- and a tile of sites may be taken through each of them by a different wave at
// the same time.  A launch whose tiles do not fill the chip a few times over (the 25-125 k sites an 8-way split of
// the BASELINE alignments leaves a GPU, real protein data) hands out (tile, segment) pairs instead of tiles: twice
// the work items of half the length, so the time of a launch with fewer tiles than wave slots -- one tile's serial
// walk of the list, ~1 us per op whatever the site count -- halves, and the last round's idle slots shrink with the
// items.  The reference has no counterpart (its cost per op is proportional to the sites, partials.c:177-213).
// Each segment is a plan of its own (order, slots, header records); reload sources, pair tables and character rows
// are numbered across the segments.  pllhip_fused_segments is host logic (CPU tests: tests/test_host.py).
struct FusedSeg
{
  unsigned int rec_first;   // the segment's two header records begin here (in records)
  unsigned int nops;
  unsigned int first_batch; // the batch of character rows its first ops use
  unsigned int pad;
};
#define PLLHIP_FUSED_MAX_SEGS 8u

// what the offsets of a FusedRec are relative to (kernel argument)
struct FusedBases
{
  const double * pmat;
  const double * pairtab;
  const unsigned long long * rowtab; // [batch][64]: the address each lane fetches its 16 bytes of tip characters from (+ site)
  const struct FusedSrc * srcs;      // reload sources, numbered across the segments
  const FusedSeg * segs;             // [nsegs] (nsegs == 1: not read, the kernel's own arguments say it all)
  unsigned int nsegs;
};
// what the edge epilogue of the list kernel reads and writes (EDGE instantiations only)
struct FusedEdgeArgs
{
  const double * freqs;                  // [rate_matrices][4]
  const double * rate_weights;           // [rate_cats]
  const unsigned int * pattern_weights;  // [sites + slack]
  double * terms;                        // [sites + PLLHIP_TAIL_SITES]: weighted per-site lnL of the edge
  unsigned int freqs_off[4];             // byte offsets of each category's frequencies in `freqs`
};

// (The planner is host logic and needs no device: what it must know of the partition is here.)
struct FusedGeom
{
  size_t nclv;            // CLV slots (tips + clv_buffers)
  size_t nsc;             // scale buffers
  unsigned int tips;
  bool pattern_tip;       // tips are character rows, not CLVs
  const unsigned char * as_tip = nullptr; // per CLV index: a deferred cherry -- an operand without a slot, like a tip
  bool is_tip(unsigned int clv_index) const { return (pattern_tip && clv_index < tips) || (as_tip && as_tip[clv_index]); }
};

// The edge evaluation a list launch also computes the per-site terms of (pllhip_ctx::edge_hint): a pseudo-op at
// position `count` that reads the two CLVs and their counts and writes no CLV.  In: the request resolved into
// addresses.  Out (pllhip_fused_plan): where the kernel finds the operands when the op loop has ended.
struct FusedEdge
{
  unsigned int parent_clv, child_clv;
  int parent_scaler, child_scaler;
  const double * parent, * child;          // the two CLVs in HBM
  const unsigned int * pscaler, * cscaler; // their scale buffers, nullptr none
  const double * pmat;                     // the edge's P-matrix
  bool deferred_before[2], pinned[2];      // {parent, child}: what pllhip_fused_edge_end_stored asks of an end
  FusedOp op;                              // out: lslot / rslot, lsc_slot / rsc_slot, what is reloaded (parent "left", child "right")
};

// Order the list, assign slots.  args/kinds are resolve_op's results per op.  Returns 0 and
// fills plan (one entry per op, in the order the kernel runs them) and *reloads (operands copied
// back from HBM), 1 if the list is of a shape the kernel does not take (the caller then
// launches per level), < 0 on error.
int pllhip_fused_plan(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args,
                      const int * kinds, unsigned int count, unsigned int nslots,
                      std::vector<FusedOp> & plan, unsigned int * reloads, const FusedExtra * extra = nullptr,
                      FusedEdge * edge = nullptr);

// Which tip-tip ops of a list are DEFERRED (not run) and what must be materialised before the list.
// Pure host logic on indices (tests/test_host_deferred_plan.py through pllhip_fused_plan_dry_deferred).
//   old_deferred[i] / old_scaler[i]: CLV i is deferred by an earlier call, with that scale buffer (-1 none)
//   pinned[i]: never deferred.  All three may be nullptr.
// Out: defer[k] = 1: op k is deferred; as_tip[i] = 1: CLV i is a gathered operand of this list (deferred now or
// before); materialise: CLVs deferred earlier that the list touches in a way a table cannot serve; dropped: CLVs
// deferred earlier that the list overwrites before reading (their deferral ends without the bytes).
struct FusedDeferral
{
  std::vector<unsigned char> defer, as_tip;
  std::vector<unsigned int> materialise, dropped;
};
void pllhip_fused_deferral(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                           const unsigned char * old_deferred, const int * old_scaler, const unsigned char * pinned,
                           FusedDeferral & out);
// May CLV `clv` be an end of the edge a list launch forms the terms of?  Only an ordinary CLV whose bytes are in HBM
// when the list has run: no tip, no cherry the list defers or reads from a table (geom.as_tip), no CLV whose address
// was handed out, and none that an earlier call left deferred -- unless this list stores it first (dd.materialise) or
// overwrites it with an ordinary op (dd.dropped).  ONE rule for pllhip_update_partials and pllhip_fused_plan_dry_edge.
bool pllhip_fused_edge_end_stored(const FusedGeom & geom, const FusedDeferral & dd, unsigned int clv,
                                  bool deferred_before, bool pinned);
// Which gathered-gathered (kind 3) parents of a planned list are left UNSTORED (pair products: deferred.hip).  The
// value needs no other CLV -- two factor tables, tip rows, the op's own counts -- so it can be formed later, and in a
// full traversal nothing reads the bytes: the one reader takes the value from the wave's slot.  An op qualifies if
//   - the list treats its parent the way a tree does (the cherries' rule): written once, read only afterwards and with
//     the op's own scale buffer or none, that buffer written by no other op and read with no other CLV, not pinned;
//   - the finished plan keeps the parent in a slot, and no op of the plan reloads it from HBM;
//   - it is read by at least one op of the list (a last op, a root, is stored);
//   - it is not an end of `edge` (the hinted evaluation, folded or not: pllhip_fused_edge_end_stored wants bytes).
// `ops` / `count`: the list the plans were made of (FusedOp::list_pos).  Sets FusedOp::unstored in `plans`, returns how
// many.  ONE rule, applied by pllhip_fused_plan_walk alone; its caller decides whether the instance may leave anything
// unstored at all.
unsigned int pllhip_fused_unstored(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                   std::vector<std::vector<FusedOp>> & plans, const FusedEdge * edge,
                                   const unsigned char * pinned);
// Which parents over two QUADS stay unstored (quad products: deferred.hip).  A walked op qualifies if it is kind 3 with
// a folded product on both sides, both read as quads (taken[segment][2 pos + side], what pllhip_fused_quad_decide made of
// the finished plan), and it passes every condition pllhip_fused_unstored puts on a pair product -- the same code.  Its
// value at a site is Qa[class a] * Qb[class b], two rows of the launch's two quad tables, times 2^256 where its own
// scaling test fired: no other CLV.  The decision follows the plan and the quads'.  `ops` / `count`: the list `plans`
// were made of (a folded walk: FusedWalk::fl).  Sets FusedOp::unstored on those ops (no other op's mark is touched),
// returns how many.  ONE rule for pllhip_launch_fused and pllhip_fused_plan_dry_quad_products.
unsigned int pllhip_fused_quad_products(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                        std::vector<std::vector<FusedOp>> & plans,
                                        const std::vector<std::vector<unsigned char>> & taken, const FusedEdge * edge,
                                        const unsigned char * pinned);
// Which unstored pair products of a planned list are FOLDED into their reader: not walked at all, the reader forms the
// product from the two gathered factors itself.  A parent pllhip_fused_unstored marked is folded if
//   - exactly one op of the list reads it, on one side only;
//   - that reader is an inner-inner op of the list (kinds[] 0): its other side is another folded product, or a slot.
// (A reader whose other side is a single gathered factor keeps today's treatment: its product is walked, unstored.)
// Sets fold[k] = 1 per op of the list to fold, returns how many -- 0 also where fewer than two ops would be left to
// walk (a list kernel wants two).  ONE rule, applied by pllhip_fused_plan_walk alone, which then plans the list once
// more without the folded ops (pllhip_fused_fold_list).
// quads: the same rule for the unstored QUAD products of a folded walk (pllhip_fused_quad_products' marks: kind-3 ops
// with a product on both sides) -- the pair products walked unstored next to them are left as they are.
unsigned int pllhip_fused_fold(const pllhip_op_t * ops, const int * kinds, unsigned int count,
                               const std::vector<std::vector<FusedOp>> & plans, std::vector<unsigned char> & fold,
                               bool quads = false);
// The list without the ops fold[] marks, as the planner is to see it: `where` (kept op -> op of the list), the kept
// ops, their args / kinds / extras with every reader's folded side turned into a product operand (FusedExtra::prod --
// to the planner a gathered side: as_tip[parent] is set for every folded parent), and rows (4 per kept op -> 8: tip
// index + 1 of the rows of its up to four factors).  extras / rows: of the list (rows may be nullptr: dry).
// quads: the list is a folded walk's (FusedWalk::fl: rows come eight per op, extras hold products) and the folded ops
// are quad products: a reader's folded side gets bit 8 and names no rows and no factors (FusedOp::q: filled from the
// plan before, pllhip_fused_quad_fold_walk).
struct FusedFoldList
{
  std::vector<unsigned int> where;
  std::vector<pllhip_op_t> ops;
  std::vector<PartialsArgs> args;
  std::vector<int> kinds;
  std::vector<FusedExtra> extras;
  std::vector<unsigned char> as_tip;
  std::vector<unsigned int> rows8;
  std::vector<unsigned int> prod_op; // 2 per kept op: the op of the list folded into side 0 / 1 of it, + 1 (0: none)
};
void pllhip_fused_fold_list(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                            const FusedExtra * extras, const unsigned int * rows4, unsigned int count,
                            const std::vector<unsigned char> & fold, FusedFoldList & out, bool quads = false);
// slots per wave with 2 (8 waves per CU) or 3 (12 waves) workgroups per CU
unsigned int pllhip_fused_slots_for(unsigned int rate_cats, bool rate_scalers, unsigned int workgroups_per_cu);
unsigned int pllhip_fused_slots(const pllhip_ctx * c, unsigned int workgroups_per_cu);
// The list as up to `max_segments` independent sub-lists of at least two ops each: seg_of[i] = segment of op i
// (segment 0 the longest; ops keep their relative order within a segment).  Components -- ops connected through a
// buffer one of them writes -- are dealt to the segments longest first, each to the segment that is shortest then.
// Returns the number of segments (1: the list does not split).
unsigned int pllhip_fused_segments(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                   unsigned int max_segments, std::vector<unsigned int> & seg_of);
// One plan per segment (both whole-list kernels): pllhip_fused_plan of the sub-list seg_of marks -- nsegs == 1: of the
// list itself, in place --, list_pos in the caller's numbering, *reloads summed.  Ends at the first plan that is not 0.
int pllhip_fused_plan_segments(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                               const FusedExtra * extra, unsigned int count, const unsigned int * seg_of, unsigned int nsegs,
                               unsigned int nslots, std::vector<std::vector<FusedOp>> & plans, unsigned int * reloads);

// The 4-state list driver: ONE rule, called by pllhip_fused_plan_walk alone.  The list is segmented and planned at each
// of slot_counts[] in turn until one is taken -- 12 waves per CU, else 8; segments refused at every slot count: once
// more as one list.  Then, with an `edge` and one segment: once more at the slot count taken with the edge as a
// pseudo-op, if both ends pass pllhip_fused_edge_end_stored; a fold the planner refuses leaves the unfolded plan.
// Returns pllhip_fused_plan's codes.
struct FusedListPlan
{
  std::vector<std::vector<FusedOp>> plans; // one per segment
  unsigned int nslots = 0, taken = 0;      // the slot count taken and its position in slot_counts[]
  unsigned int reloads = 0;
  bool folded = false;                     // plans[0] ends in the edge pseudo-op: edge->op says where its operands are
};
int pllhip_fused_plan_list(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                           const FusedExtra * extra, unsigned int count, unsigned int max_segments,
                           const unsigned int * slot_counts, unsigned int nslot_counts, FusedEdge * edge,
                           const FusedDeferral & dd, FusedListPlan & out);

// The whole preparation of a 4-state list, ONE sequence for pllhip_update_partials (real addresses) and the dry entry
// points pllhip_fused_plan_dry_deferred / _edge / _unstored / _folded (fake ones; no device, no callback):
//   1. the list is planned (pllhip_fused_plan_list, `edge` offered where given);
//   2. may_unstore: pllhip_fused_unstored marks the parents that stay unstored;
//   3. may_fold, and something is unstored: pllhip_fused_fold picks those its reader forms, pllhip_fused_fold_list builds
//      the list without them, and that list is planned once more -- the edge offered only where the first plan had one
//      segment (a list in segments stays without, however short its segments have become).  A second plan the planner
//      refuses, or one of fewer than two ops, leaves the first;
//   4. a second plan taken: pllhip_fused_unstored once more, on what is left.
// ops / args / kinds / extras (may be nullptr) / rows4 (four per op: tip index + 1 of the rows of its two gathered
// factors; may be nullptr: dry): the ops the kernel is to run, after deferral.  The arrays must outlive the result,
// which refers to them.  Returns the first plan's code (pllhip_fused_plan's); < 0 also for an error of the second.
struct FusedWalk
{
  FusedListPlan plan; // the plan to launch, and its edge (plan.folded: edge.op says where the epilogue's operands are)
  FusedEdge edge;
  // a folded plan replaced the first: the first is kept, its unstored marks standing, should the launch not take the
  // second (more character batches or tables than it encodes) -- take_first()
  bool replanned = false;
  FusedListPlan first_plan;
  FusedEdge first_edge;
  std::vector<unsigned char> fold; // per op of the list: folded, not walked (all 0 unless replanned)
  FusedFoldList fl;                // replanned: the list `plan` was made of
  unsigned int nunstored = 0;      // walked parents `plan` leaves unstored
  unsigned int nfolded = 0;        // folded ones (not walked, unstored too)
  unsigned int first_nunstored = 0;
  const pllhip_op_t * list_ops = nullptr;
  const unsigned int * list_rows4 = nullptr;

  // What an op of `plan` stands for: its position in the list handed over, the op itself, the four rows its parent is
  // kept with where it stays unstored (nullptr: dry), and the op of the list folded into side s of it (nullptr: none).
  unsigned int pos_in_list(const FusedOp & f) const { return replanned ? fl.where[f.list_pos] : (unsigned int)f.list_pos; }
  const pllhip_op_t & op_of(const FusedOp & f) const { return list_ops[pos_in_list(f)]; }
  const unsigned int * rows_of(const FusedOp & f) const { return list_rows4 ? list_rows4 + 4 * (size_t)pos_in_list(f) : nullptr; }
  const pllhip_op_t * folded_into(const FusedOp & f, int s) const
  {
    const unsigned int from = replanned && f.prod[s] ? fl.prod_op[2 * (size_t)f.list_pos + s] : 0u;
    return from ? list_ops + (from - 1) : nullptr;
  }
  // the launch did not take the folded plan: the first one again
  void take_first()
  {
    plan = std::move(first_plan);
    edge = first_edge;
    replanned = false;
    fold.assign(fold.size(), 0);
    nunstored = first_nunstored;
    nfolded = 0;
  }
};
int pllhip_fused_plan_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                           const FusedExtra * extras, const unsigned int * rows4, unsigned int count,
                           unsigned int max_segments, const unsigned int * slot_counts, unsigned int nslot_counts,
                           const FusedEdge * edge, const FusedDeferral & dd, const unsigned char * pinned,
                           bool may_unstore, bool may_fold, FusedWalk & out);

// The quad fold (DESIGN.md 2.0 "Folded quad products"), behind pllhip_fused_plan_walk and the launch's choice of quads:
// the unstored quad products of a folded walk that exactly one inner-inner op reads are not walked either -- their
// reader gathers the two quads and forms the product itself (pllhip_fused_fold, quads).  The list without them
// (pllhip_fused_fold_list) is planned once more by pllhip_fused_plan_list, at the slot count the plan before took.
// ops / args / kinds / extras / rows8 / count: the list `plans` were made of (FusedWalk::fl); plans: the plan before,
// with pllhip_fused_quad_products' marks; edge: its edge where it ends in the pseudo-op, else nullptr -- the new plan
// is taken only if it keeps it.  Every op of the new plan is given what its op had in the plan before (unstored, keep,
// pkeep) and every folded side the factors of the op folded into it (FusedOp::q, qkeep); a walked op that was
// unstored must still be kept in a slot and never reloaded.  Returns 0: out.plan is to be launched; 1: nothing folds,
// or the planner does not take the list -- the plan before stands; < 0 on error.
struct FusedQuadFold
{
  std::vector<unsigned char> fold; // per op of the list: folded, not walked
  FusedFoldList fl;                // the list `plan` was made of
  FusedListPlan plan;
  FusedEdge edge;
  unsigned int nfolded = 0;
};
int pllhip_fused_quad_fold_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                                const FusedExtra * extras, const unsigned int * rows8, unsigned int count,
                                const std::vector<std::vector<FusedOp>> & plans, unsigned int max_segments, unsigned int nslots,
                                const FusedEdge * edge, const FusedDeferral & dd, FusedQuadFold & out);

// ---- The 20-state list (partials_aa_fused.hip) before anything is encoded: what each op is to the kernel, what the
// scaling certificate makes of it, the list the kernel walks.  Indices and numbers only -- ONE rule for
// pllhip_aa_fused_update (real addresses) and pllhip_aa_list_plan_dry (fake ones; tests/test_host_aa_list_plan.py).
constexpr unsigned int PLLHIP_AA_FUSED_SLOTS = 5; // values a wave of k_aa_fused keeps in registers
enum AaOpClass
{
  AA_OP_II = 0,       // inner-inner, on the matrix cores
  AA_OP_TI = 1,       // tip-inner
  AA_OP_TT_AHEAD = 2, // tip-tip, run ahead of the list kernel (PLLHIP_AA_TT_INSIDE=0)
  AA_OP_LOOKUP = 3,   // an inner-inner op over two tip-tip results of this list, or a tip-inner op over one: two table rows
  AA_OP_TT_LIST = 4   // tip-tip, in the list: a lookup over the two tip tables, or one row of its pair table
};
// what the planner and the kernel take a walked op for: 0 inner-inner, 1 tip-inner, 2 no inner operand (a "lookup")
inline int pllhip_aa_walk_kind(int cls) { return cls >= AA_OP_TT_AHEAD ? 2 : cls; }
struct AaListClasses
{
  std::vector<int> cls;                     // AaOpClass per op
  std::vector<std::pair<int, int>> lk_kids; // a lookup's producing ops {of child 1 (-2: a tip-inner lookup, no producer), of the inner child}
  unsigned int lookups = 0;
  bool any_scaler = false;
};
// kinds[i]: resolve_op's plain kind (0 / 1 / 2); scales[i] != 0: op i has a scale buffer.  At most `lookups_max`
// lookups, the first eligible ops in list order.  Returns 1 -- the list runs per level -- for a tip-tip op whose parent
// or scale buffer an earlier op of the list touched (tip-tip ops read tips only: they may run ahead of everything
// only if nothing before them wrote or read what they write).
int pllhip_aa_list_classify(const FusedGeom & geom, const pllhip_op_t * ops, const int * kinds, const int * scales,
                            unsigned int count, unsigned int lookups_max, bool tt_inside, AaListClasses & out);
// The scaling certificate's bounds (ctx.hpp): a bound on every op's relative difference from the
// reference's value -- its operands' bounds plus PLLHIP_CERT_OP_ERR when anything at or below it is a tip-inner op on
// the matrix cores --, which ops therefore test, and the window they test with.  incoming: the bound an earlier call
// left on each CLV (nullptr: none anywhere).  ti_mfma: tip-inner mat-vecs on the matrix cores are wanted; list_ti_mfma:
// and had -- not by a list that overwrites an operand it read from an earlier call (it could not be run again), nor,
// second attempt, when the bounds would outgrow the widest window.
struct AaListCert
{
  std::vector<unsigned char> op_inexact; // per op: its scaling test also looks for the window
  bool list_ti_mfma = false, too_wide = false;
  int cert_kind = 0;                     // 0 nothing tests; 1 a trip runs the list again; 2 the bounds are inherited only
  double window = 0.0;
  std::vector<std::pair<unsigned int, double>> ext_marks, out_marks; // (CLV, bound): read from earlier calls, in the
                                                                     // order first read; left by the list, by index
};
void pllhip_aa_list_cert(const FusedGeom & geom, const pllhip_op_t * ops, const int * cls, unsigned int count,
                         const double * incoming, bool ti_mfma, AaListCert & out);
// The list the kernel walks: every op but the tip-tip ops ahead of it, segmented (pllhip_fused_segments), ordered and
// given slots by the planner (a lookup or a tip-tip op has no inner operand: "tip-tip" to the planner).
struct AaListWalk
{
  std::vector<unsigned int> ahead;           // the tip-tip ops ahead of the list, grouped: without a scale buffer first
  std::vector<int> orig;                     // walked op -> op of the caller's list
  std::vector<FusedOp> plan;                 // the segments' plans one after the other; list_pos: the walked op
  std::vector<unsigned int> seg_first, seg_n;
  // The left block of op i is staged by the four waves, a part each, while they run op i - 2, and the barrier that
  // tells a wave that everybody's part has landed is barrier A of op i - 1 -- which a lookup does not have.  An
  // inner-inner op whose predecessor in its segment's cyclic walk is a lookup or a tip-tip op therefore begins with
  // a barrier of its own (AF_SYNC_LEFT): without it, over runs of tens of barrier-free ops the waves drift apart by
  // whole ops, and the op read its left block a few hundred cycles after the waves had last met.
  std::vector<unsigned char> sync_left;      // per position of `plan`
  unsigned int nsegs = 1, reloads = 0;
};
// Returns 0; 1 for a list of nothing but tip-tip ops ahead, or one the planner does not take; < 0 on error.
int pllhip_aa_list_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * cls,
                        const int * scales, unsigned int count, unsigned int max_segments, unsigned int nslots,
                        AaListWalk & out);
// pllhip_aa_list_kinds' eight numbers: ops, tip-tip ahead of the list, tip-tip in the list, lookups, inner-inner on the
// matrix cores, tip-inner on the matrix cores, tip-inner on the vector unit, operands reloaded
void pllhip_aa_list_kinds_of(const int * cls, unsigned int count, bool list_ti_mfma, unsigned int reloads,
                             unsigned int * out8);

// Quad products (deferred.hip): what the launch needs to apply pllhip_fused_quad_products once it has picked the quads
// -- the list the plans were made of, the hinted edge (folded or not), the pinned CLVs --, and what it left unstored:
// the CLV and scale buffer of each such op, its two quad rows (their places in the pool of rows) and its place in the
// pool of kept quad tables.
struct FusedQuadProducts
{
  FusedGeom geom;
  const pllhip_op_t * ops = nullptr;
  unsigned int count = 0;
  const FusedEdge * edge = nullptr;
  const unsigned char * pinned = nullptr;
  std::vector<pllhip_ctx::deferred_clv> left; // out: their records
  // the quad fold (pllhip_fused_quad_fold_walk): the rest of the list the plans were made of, and how it was planned;
  // out: the plan launched in place of the one handed over (nfolded != 0), whose parents `left` has as UNSTORED_QUAD_FOLDED
  bool fold = false;
  const PartialsArgs * args = nullptr;
  const int * kinds = nullptr;
  const FusedExtra * extras = nullptr;
  const unsigned int * rows8 = nullptr;
  unsigned int max_segments = 1;
  const FusedDeferral * dd = nullptr;
  FusedQuadFold folded;
  unsigned int nfolded = 0;
};
// Table reuse (DESIGN.md 2.0 "Table reuse"): which table jobs of the kept plan a launch runs.  THE staleness rule, host
// logic over arrays (pllhip_table_reuse_dry: tests/test_host_table_reuse.py): a job is stale where `all` says so -- a new
// plan, pllhip_tables_mark_stale, reuse switched off -- or a matrix it names was written after the tables were last
// built (written[m] > built; PLLHIP_JOB_MAT_UNKNOWN: always).  A record of kind 5 is the second half of the quad ahead
// of it: its matrices are in that record's reads, and it is no job.  mask: bit i set where the workgroups of job record
// i run -- a by-value argument of both table kernels; a list of more records than it holds runs all of them or none
// (the kernels do not test a record past the mask).  out4 = {jobs that run, jobs skipped, 1 where a job of kinds 0 - 3
// runs: k_dna_pair_tables is launched, 1 where a quad runs: k_dna_quad_tables is}.
constexpr unsigned int PLLHIP_TABLE_MASK_WORDS = 16u, PLLHIP_TABLE_MASK_JOBS = 64u * PLLHIP_TABLE_MASK_WORDS;
struct FusedStaleMask
{
  unsigned long long w[PLLHIP_TABLE_MASK_WORDS];
};
inline void pllhip_fused_stale_jobs(const FusedJobReads * jobs, unsigned int njobs, const unsigned long long * written,
                                    unsigned int nmats, unsigned long long built, bool all, FusedStaleMask & mask,
                                    unsigned int * out4)
{
  auto is_stale = [&](const FusedJobReads & j) {
    for (unsigned int m : j.mat)
      if (m != PLLHIP_JOB_MAT_NONE && (m >= nmats || written[m] > built)) return true;
    return false;
  };
  bool any = false;
  for (unsigned int i = 0; i < njobs && !any; ++i) any = jobs[i].kind != 5u && is_stale(jobs[i]);
  if (any && njobs > PLLHIP_TABLE_MASK_JOBS) all = true;
  memset(&mask, 0, sizeof(mask));
  out4[0] = out4[1] = out4[2] = out4[3] = 0u;
  for (unsigned int i = 0; i < njobs; ++i)
  {
    if (jobs[i].kind == 5u) continue;
    if (!all && !is_stale(jobs[i]))
    {
      ++out4[1];
      continue;
    }
    ++out4[0];
    out4[jobs[i].kind == 4u ? 3 : 2] = 1u;
    if (i < PLLHIP_TABLE_MASK_JOBS) mask.w[i >> 6] |= 1ull << (i & 63u);
  }
}
// the kernels' side of it: do the workgroups of job record i run (a scalar test of a kernel argument)
__host__ __device__ __forceinline__ bool pllhip_fused_job_runs(const FusedStaleMask & mask, unsigned int i)
{
  return i >= PLLHIP_TABLE_MASK_JOBS || ((mask.w[i >> 6] >> (i & 63u)) & 1ull) != 0ull;
}

// encode and launch: one plan per segment
int pllhip_launch_fused(pllhip_ctx * c, const std::vector<std::vector<FusedOp>> & plans, unsigned int nslots,
                        const std::vector<FusedPairJob> * keep_jobs = nullptr, const FusedEdge * edge = nullptr,
                        FusedQuadProducts * quad_products = nullptr);
int pllhip_relaunch_fused(pllhip_ctx * c); // the same op list as in the previous whole-list call of this context

#endif
