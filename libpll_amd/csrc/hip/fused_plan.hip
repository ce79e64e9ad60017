// fused_plan.hip -- the planner of the whole-list kernels (partials_fused.hip, 4 states; partials_aa_fused.hip, 20):
// host logic on op lists and indices.  No device, no context, no kernel: the *_dry entry points run all of it in the
// CPU tests (tests/test_host.py, test_host_deferred_plan.py, test_host_edge_fold_plan.py).
//   op order  any order that respects the list's read/write hazards on CLV and scale buffer indices is equivalent; the
//             list is re-ordered depth-first, heavier subtree first (Sethi-Ullman), which bounds the number of live
//             values by the tree's Strahler number (5 for a balanced 64-taxon tree, 6 for 128 taxa, not the 32 / 64
//             of a level-by-level list)
//   slots     a value keeps its LDS slot until its last reader in the list has run (assign_slots_reload)
//   driver    cherries deferred, segments, 12 waves per CU or 8, the edge pseudo-op: pllhip_fused_plan_list
//   20 states what comes before the planner there: every op's class (pllhip_aa_list_classify), the scaling certificate's
//             bounds (pllhip_aa_list_cert), the list the kernel walks and its barriers (pllhip_aa_list_walk);
//             pllhip_aa_list_plan_dry runs the three (tests/test_host_aa_list_plan.py, test_gpu_aa_list_plan.py)
#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory_resource>
#include <vector>

#include "ctx.hpp"
#include "partials_fused.hpp"

namespace
{
// (round 4) The planner's many small lists -- hazard predecessors, readers per buffer, uses per value -- come from a
// bump allocator over a per-thread buffer: as std::vectors on the heap they were most of its time (0.32 us per op,
// 20 us for BASELINE config 2's 62-op list, 75 us for a 198-op list; VERDICT r3 Weak 6: tree search hands over a new
// list almost every call).
typedef std::pmr::vector<unsigned int> PlanList;
typedef std::pmr::vector<PlanList> PlanLists;
struct Node
{
  int raw[2] = {-1, -1};          // producers of the two children within the list (-1: outside)
  int sraw[2] = {-1, -1};         // writers of the two child scale buffers within the list
  unsigned int need = 1;          // Sethi-Ullman number of the subtree rooted here
};
}

// slots per wave when `wgs` workgroups of four waves share a CU's LDS: 64 KB per workgroup
// for two (8 waves per CU), 52 KB for three (12 waves: better latency hiding, one slot less)
unsigned int pllhip_fused_slots_for(unsigned int R, bool rate_scalers, unsigned int wgs)
{
  // 64 KB per workgroup of four waves: 16 KB per wave minus the matrix block
  const size_t per_slot = pllhip_fused_slot_size(R, rate_scalers).bytes();
  const size_t pmat = (size_t)R * 16 * sizeof(double); // one matrix at a time (stage_rows)
  // (four workgroups -- 16 waves of 128 registers, four slots -- were measured for short lists in round 3 and are
  // slower than three at every list length: 2 / 3 / 5 / 7 / 15 ops 257 / 286 / 335 / 282 / 421 us against 226 / 260 /
  // 310 / 246 / 411; the variant spills seven registers)
  // (1 KB of it is the wave's character batch: the sixth slot of four rate categories on twelve waves went for it)
  const size_t budget = wgs >= 3 ? 13312 : 16384;
  return (unsigned int)((budget - pmat - PLLHIP_FUSED_BATCH_BYTES) / per_slot);
}

// Slot assignment: every inner operand is read from a slot.  A value whose
// slot was taken away (or that an earlier call wrote) is copied back from HBM into a slot by
// the kernel's reload() at the top of the op BEFORE its reader; that slot must be free from
// then on (not read by that op, not its parent's).  Belady's rule decides who gives a slot up:
// the live value whose next reader is farthest away.
static int assign_slots_reload(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args,
                               const int * kinds, unsigned int count, unsigned int nslots,
                               const std::vector<unsigned int> & order, const std::vector<unsigned int> & pos_of,
                               const std::vector<Node> & node, std::vector<FusedOp> & plan,
                               unsigned int * reloads_out, std::pmr::memory_resource * pool, const FusedExtra * extra,
                               FusedEdge * edge, const int * edge_raw, const int * edge_sraw)
{
  // the edge pseudo-op (FusedEdge): position `count`, list index `count` -- it reads two values and writes none
  const unsigned int total = count + (edge ? 1u : 0u);
  // inner operands of the op at each position: producing list op (-1: written by an earlier
  // call), its HBM address, the HBM address of the counts the reader passes with it, and the
  // list op that wrote those counts
  struct Operand { int w; const double * hbm; const unsigned int * sc; int sw; };
  auto operands = [&](unsigned int i, Operand (&o)[2]) {
    o[0] = o[1] = Operand{-2, nullptr, nullptr, -1}; // -2: no such operand (a tip)
    if (i == count)
    {
      o[0] = Operand{edge_raw[0], edge->parent, edge->pscaler, edge_sraw[0]};
      o[1] = Operand{edge_raw[1], edge->child, edge->cscaler, edge_sraw[1]};
    }
    else if (kinds[i] == 0)
    {
      o[0] = Operand{node[i].raw[0], args[i].left, args[i].lscaler, node[i].sraw[0]};
      o[1] = Operand{node[i].raw[1], args[i].right, args[i].rscaler, node[i].sraw[1]};
    }
    else if (kinds[i] == 1)
    {
      const int inner = geom.is_tip(ops[i].child1_clv) ? 1 : 0;
      o[1] = Operand{node[i].raw[inner], args[i].right, args[i].rscaler, node[i].sraw[inner]};
    }
  };
  PlanLists uses(count, pool); // positions at which each list value is read
  for (unsigned int pos = 0; pos < total; ++pos)
  {
    Operand o[2];
    operands(pos < count ? order[pos] : count, o);
    if (o[0].w >= 0) uses[o[0].w].push_back(pos);
    if (o[1].w >= 0 && o[1].w != o[0].w) uses[o[1].w].push_back(pos);
  }
  std::vector<unsigned int> next_use(count, 0);
  std::vector<int> slot_of(count, -1);
  std::vector<int> free_slots;
  for (int s = (int)nslots - 1; s >= 0; --s) free_slots.push_back(s);
  std::vector<unsigned int> live;          // list values that hold a slot
  std::vector<int> oneshot, oneshot_next;  // slots of operands from earlier calls (of this op / the next): free after their one reader
  unsigned int reloads = 0;
  const unsigned int NEVER = ~0u;
  auto next_read = [&](unsigned int v) { return next_use[v] < uses[v].size() ? uses[v][next_use[v]] : NEVER; };
  // a slot that may be written from position `pos` on: a free one, else that of the live
  // value read farthest in the future -- but not before pos + 2 (its own reload is issued at
  // the top of the op before its reader and needs a slot free by then)
  auto take_slot = [&](unsigned int pos) -> int {
    if (!free_slots.empty())
    {
      const int s = free_slots.back();
      free_slots.pop_back();
      return s;
    }
    int victim = -1;
    unsigned int far = 0;
    for (unsigned int v : live)
    {
      const unsigned int u = next_read(v);
      if (u != NEVER && u >= pos + 2 && u >= far)
      {
        far = u;
        victim = (int)v;
      }
    }
    if (victim < 0) return -1;
    const int s = slot_of[victim];
    slot_of[victim] = -1;
    live.erase(std::find(live.begin(), live.end(), (unsigned int)victim));
    return s;
  };
  // operands of the op at position `pos` that are not in a slot: reloaded at the top of
  // position pos - 1 (`at`; the kernel's prologue for pos 0)
  auto place_reloads = [&](unsigned int pos, unsigned int at) -> int {
    const unsigned int i = pos < count ? order[pos] : count;
    FusedOp & f = pos < count ? plan[pos] : edge->op;
    Operand o[2];
    operands(i, o);
    for (int side = 0; side < 2; ++side)
    {
      const Operand & x = o[side];
      if (x.w == -2) continue;
      if (side == 1 && x.w >= 0 && x.w == o[0].w) continue; // the same value twice: one slot
      if (x.w >= 0 && (pos_of[x.w] >= at || slot_of[x.w] >= 0)) continue; // still to come, or in a slot
      if (x.w >= 0 && pos_of[x.w] + 2 >= pos) return 1; // (cannot happen: evicted values are read later)
      const int s = take_slot(at);
      if (s < 0) return 1;
      ++reloads;
      const unsigned int * counts = nullptr;
      if (x.w >= 0)
      {
        // a value of this list: its counts are those its producer wrote, whoever reads it
        counts = args[x.w].pscaler;
        slot_of[x.w] = s;
        live.push_back((unsigned int)x.w);
      }
      else
      {
        // written by an earlier call: the counts the reader passes, which no op of this list
        // may have rewritten shortly before
        if (x.sc && x.sw >= 0 && pos_of[x.sw] + 2 >= pos) return 1;
        counts = x.sc;
        oneshot_next.push_back(s);
      }
      if (side == 0) { f.left_hbm = x.hbm; f.lsc_hbm = counts; f.lslot = s; f.dma_flags |= 1; }
      else { f.right_hbm = x.hbm; f.rsc_hbm = counts; f.rslot = s; f.dma_flags |= 2; }
    }
    return 0;
  };

  plan.resize(count);
  for (unsigned int pos = 0; pos < count; ++pos)
  {
    const unsigned int i = order[pos];
    const PartialsArgs & a = args[i];
    FusedOp & f = plan[pos];
    memset(&f, 0, sizeof(f));
    f.parent = a.parent;
    f.ltip = a.ltip;
    f.rtip = a.rtip;
    f.lmat = a.lmat;
    f.rmat = a.rmat;
    f.pscaler = a.pscaler;
    f.kind = kinds[i];
    f.list_pos = (int)i;
    f.lslot = f.rslot = f.pslot = f.lsc_slot = f.rsc_slot = -1;
    if (extra)
    {
      f.g[0] = extra[i].g[0];
      f.g[1] = extra[i].g[1];
      for (int s = 0; s < 2; ++s)
      {
        f.g2[s] = extra[i].g2[s];
        f.prod[s] = extra[i].prod[s];
        f.pkeep[s][0] = extra[i].pkeep[s][0];
        f.pkeep[s][1] = extra[i].pkeep[s][1];
      }
    }
  }
  if (edge)
  {
    memset(&edge->op, 0, sizeof(edge->op));
    edge->op.kind = PLLHIP_FUSED_KIND_EDGE;
    edge->op.list_pos = (int)count;
    edge->op.lslot = edge->op.rslot = edge->op.pslot = edge->op.lsc_slot = edge->op.rsc_slot = -1;
  }
  if (place_reloads(0, 0)) return 1;
  oneshot.swap(oneshot_next);
  for (unsigned int pos = 0; pos < total; ++pos)
  {
    const unsigned int i = pos < count ? order[pos] : count;
    FusedOp & f = pos < count ? plan[pos] : edge->op;
    // top of the op: the next op's missing operands are requested into slots free NOW
    if (pos + 1 < total && place_reloads(pos + 1, pos)) return 1;
    Operand o[2];
    operands(i, o);
    for (int side = 0; side < 2; ++side)
    {
      const Operand & x = o[side];
      if (x.w == -2) continue;
      int & slot = side == 0 ? f.lslot : f.rslot;
      int & sc_slot = side == 0 ? f.lsc_slot : f.rsc_slot;
      if (x.w >= 0)
      {
        if (slot < 0) slot = slot_of[x.w];
        if (slot < 0) return 1;
        // counts: only those written together with the value live in its slot
        if (x.sc)
        {
          if (x.sw != x.w || x.sc != args[x.w].pscaler) return 1;
          sc_slot = slot;
        }
      }
      else
      {
        if (slot < 0) return 1; // (placed by place_reloads)
        if (x.sc) sc_slot = slot;
      }
    }
    if (pos == count) break; // (the edge pseudo-op: nothing runs after it, and it writes no value)
    // operands read for the last time give their slots back
    for (int side = 0; side < 2; ++side)
    {
      const int w = o[side].w;
      if (w < 0 || (side == 1 && w == o[0].w)) continue;
      if (next_use[w] < uses[w].size() && uses[w][next_use[w]] == pos) next_use[w]++;
      if (next_use[w] >= uses[w].size() && slot_of[w] >= 0)
      {
        free_slots.push_back(slot_of[w]);
        slot_of[w] = -1;
        live.erase(std::find(live.begin(), live.end(), (unsigned int)w));
      }
    }
    for (int s : oneshot) free_slots.push_back(s);
    oneshot.clear();
    oneshot.swap(oneshot_next);
    // the parent: a slot if it has readers -- unless its first reader is far enough away for a
    // reload (three ops: its stores must have left) and farther than every live value's next
    if (!uses[i].empty())
    {
      const unsigned int first = uses[i][0];
      bool wants = true;
      if (free_slots.empty() && first >= pos + 3)
      {
        unsigned int far = 0;
        for (unsigned int v : live)
        {
          const unsigned int u = next_read(v);
          if (u != NEVER && u >= pos + 2 && u > far) far = u;
        }
        if (first >= far) wants = false;
      }
      if (wants)
      {
        const int s = take_slot(pos);
        if (s < 0)
        {
          if (first < pos + 3) return 1;
        }
        else
        {
          f.pslot = s;
          slot_of[i] = s;
          live.push_back(i);
        }
      }
    }
  }
  *reloads_out = reloads;
  return 0;
}

int pllhip_fused_plan(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args,
                      const int * kinds, unsigned int count, unsigned int nslots,
                      std::vector<FusedOp> & plan, unsigned int * reloads_out, const FusedExtra * extra, FusedEdge * edge)
{
  static thread_local std::vector<char> arena(256 * 1024);
  std::pmr::monotonic_buffer_resource pool(arena.data(), arena.size()); // (beyond the buffer: the heap)
  std::vector<Node> node(count);
  PlanLists hard_of(count, &pool); // WAW / WAR predecessors (and scaler hazards) of each op: must run before it
  const size_t nclv = geom.nclv, nsc = geom.nsc;
  // last writer and readers-since of every CLV / scale buffer, in list order
  std::pmr::vector<int> clv_w(nclv, -1, &pool), sc_w(nsc, -1, &pool);
  PlanLists clv_r(nclv, &pool), sc_r(nsc, &pool);
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_op_t & op = ops[i];
    Node & nd = node[i];
    nd.raw[0] = clv_w[op.child1_clv];
    nd.raw[1] = clv_w[op.child2_clv];
    // (round 6: a predecessor that is one of the op's two PRODUCERS is no hazard of its own -- the usual case: a
    // child's scale buffer was written by the op that wrote the child -- and must not be walked ahead of the
    // "heavier child first" rule below.  Until then every list with scale buffers was walked child 1 first, whatever the
    // subtrees' sizes: a traversal directed at a deep edge of a balanced 64-taxon tree needed 4 operands copied back
    // from HBM with five slots and ended in a run of seven matrix ops; now none, and at most three in a row.)
    auto hard = [&](int p) {
      if (p >= 0 && (unsigned int)p != i && p != nd.raw[0] && p != nd.raw[1])
        hard_of[i].push_back((unsigned int)p);
    };
    nd.sraw[0] = op.child1_scaler >= 0 ? sc_w[op.child1_scaler] : -1;
    nd.sraw[1] = op.child2_scaler >= 0 ? sc_w[op.child2_scaler] : -1;
    hard(clv_w[op.parent_clv]);
    for (unsigned int r : clv_r[op.parent_clv]) hard((int)r);
    hard(nd.sraw[0]);
    hard(nd.sraw[1]);
    if (op.parent_scaler >= 0)
    {
      hard(sc_w[op.parent_scaler]);
      for (unsigned int r : sc_r[op.parent_scaler]) hard((int)r);
    }
    clv_w[op.parent_clv] = (int)i;
    clv_r[op.parent_clv].clear();
    clv_r[op.child1_clv].push_back(i);
    clv_r[op.child2_clv].push_back(i);
    if (op.parent_scaler >= 0)
    {
      sc_w[op.parent_scaler] = (int)i;
      sc_r[op.parent_scaler].clear();
    }
    if (op.child1_scaler >= 0) sc_r[op.child1_scaler].push_back(i);
    if (op.child2_scaler >= 0) sc_r[op.child2_scaler].push_back(i);
    const unsigned int a = nd.raw[0] >= 0 ? node[nd.raw[0]].need : 0;
    const unsigned int b = nd.raw[1] >= 0 ? node[nd.raw[1]].need : 0;
    nd.need = std::max(1u, a == b ? a + (a ? 1u : 0u) : std::max(a, b));
  }

  // depth-first order from the end of the list: hazards first, then the heavier child
  std::vector<unsigned int> order;
  order.reserve(count);
  {
    std::vector<unsigned char> state(count, 0); // 0 new, 1 open, 2 emitted
    std::vector<std::pair<unsigned int, unsigned int>> stack; // (op, next predecessor to look at)
    PlanLists & preds = hard_of; // (the two producers are appended: hazards first, then the heavier child)
    for (unsigned int i = 0; i < count; ++i)
    {
      int r0 = node[i].raw[0], r1 = node[i].raw[1];
      if (r0 >= 0 && r1 >= 0 && node[r1].need > node[r0].need) std::swap(r0, r1);
      if (r0 >= 0) preds[i].push_back((unsigned int)r0);
      if (r1 >= 0 && r1 != r0) preds[i].push_back((unsigned int)r1);
    }
    for (unsigned int root = count; root-- > 0;)
    {
      if (state[root]) continue;
      stack.push_back({root, 0});
      state[root] = 1;
      while (!stack.empty())
      {
        auto & top = stack.back();
        if (top.second < preds[top.first].size())
        {
          const unsigned int p = preds[top.first][top.second++];
          if (!state[p])
          {
            state[p] = 1;
            stack.push_back({p, 0});
          }
        }
        else
        {
          state[top.first] = 2;
          order.push_back(top.first);
          stack.pop_back();
        }
      }
    }
  }
  std::vector<unsigned int> pos_of(count);
  for (unsigned int pos = 0; pos < count; ++pos) pos_of[order[pos]] = pos;

  // the edge pseudo-op reads what the list leaves in the two CLVs and scale buffers: their LAST writers.  An end the
  // list does not keep in HBM (a tip, a deferred cherry), the same CLV twice, or a list that writes neither end: no fold
  int edge_raw[2] = {-1, -1}, edge_sraw[2] = {-1, -1};
  if (edge)
  {
    if (edge->parent_clv >= nclv || edge->child_clv >= nclv || edge->parent_clv == edge->child_clv ||
        geom.is_tip(edge->parent_clv) || geom.is_tip(edge->child_clv) ||
        edge->parent_scaler >= (int)nsc || edge->child_scaler >= (int)nsc)
      return 1;
    edge_raw[0] = clv_w[edge->parent_clv];
    edge_raw[1] = clv_w[edge->child_clv];
    if (edge_raw[0] < 0 && edge_raw[1] < 0) return 1;
    edge_sraw[0] = edge->parent_scaler >= 0 ? sc_w[edge->parent_scaler] : -1;
    edge_sraw[1] = edge->child_scaler >= 0 ? sc_w[edge->child_scaler] : -1;
  }
  const int rc = assign_slots_reload(geom, ops, args, kinds, count, nslots, order, pos_of, node, plan, reloads_out, &pool, extra,
                                     edge, edge_raw, edge_sraw);
  if (rc) return rc;
  if (pllhip_env("PLLHIP_FUSED_DEBUG"))
  {
    fprintf(stderr, "pllhip fused plan: %u ops, %u slots, %u operands reloaded from HBM\n", count, nslots, *reloads_out);
    if (atoi(pllhip_env("PLLHIP_FUSED_DEBUG")) > 1)
      for (unsigned int pos = 0; pos < count; ++pos)
      {
        const FusedOp & f = plan[pos];
        fprintf(stderr, "  %3u: op %3d kind %d  l %2d r %2d p %2d  lsc %2d rsc %2d  dma %d  hbm %p %p counts %p %p\n", pos,
                f.list_pos, f.kind, f.lslot, f.rslot, f.pslot, f.lsc_slot, f.rsc_slot, f.dma_flags,
                (const void *)f.left_hbm, (const void *)f.right_hbm, (const void *)f.lsc_hbm, (const void *)f.rsc_hbm);
      }
  }
  return 0;
}

// Which tip-tip ops a list defers (partials_fused.hpp).  A deferred CLV is served from tables only while the list
// treats it the way a tree does: written once, by that op; read after it, with the scale buffer it was cleared with (or
// none); that scale buffer written by nobody else and read with nobody else.  Anything else is materialised (a CLV
// deferred earlier) or simply not deferred (an op of this list) -- the list then sees ordinary buffers.
void pllhip_fused_deferral(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                           const unsigned char * old_deferred, const int * old_scaler, const unsigned char * pinned,
                           FusedDeferral & out)
{
  const size_t nclv = geom.nclv, nsc = geom.nsc;
  const unsigned int NONE = ~0u;
  out.defer.assign(count, 0);
  out.as_tip.assign(nclv, 0);
  out.materialise.clear();
  out.dropped.clear();
  auto true_tip = [&](unsigned int i) { return geom.pattern_tip && i < geom.tips; };
  std::vector<unsigned int> nwrites(nclv, 0), first_write(nclv, NONE), first_read(nclv, NONE);
  std::vector<unsigned int> sc_nwrites(nsc, 0), sc_first_write(nsc, NONE), sc_first_read(nsc, NONE);
  std::vector<int> cand_sc(nclv, -2);        // the scale buffer a deferred CLV i would own (-1 none, -2: no candidate)
  std::vector<int> sc_reader(nsc, -1);       // the one CLV a scale buffer is read with (-1 nobody, -2 several)
  std::vector<unsigned char> bad(nclv, 0);   // read with a scale buffer that is not its own
  for (unsigned int k = 0; k < count; ++k)
  {
    const pllhip_op_t & op = ops[k];
    ++nwrites[op.parent_clv];
    if (first_write[op.parent_clv] == NONE) first_write[op.parent_clv] = k;
    if (op.parent_scaler >= 0)
    {
      ++sc_nwrites[op.parent_scaler];
      if (sc_first_write[op.parent_scaler] == NONE) sc_first_write[op.parent_scaler] = k;
    }
  }
  for (size_t i = 0; i < nclv; ++i)
  {
    if (old_deferred && old_deferred[i]) cand_sc[i] = old_scaler ? old_scaler[i] : -1;
    if (nwrites[i] == 1)
    {
      const pllhip_op_t & op = ops[first_write[i]];
      if (true_tip(op.child1_clv) && true_tip(op.child2_clv) && !true_tip((unsigned int)i) && !(pinned && pinned[i]) &&
          !(old_deferred && old_deferred[i]))
        cand_sc[i] = op.parent_scaler;
    }
  }
  for (unsigned int k = 0; k < count; ++k)
  {
    const pllhip_op_t & op = ops[k];
    const unsigned int kid[2] = {op.child1_clv, op.child2_clv};
    const int ksc[2] = {op.child1_scaler, op.child2_scaler};
    for (int o = 0; o < 2; ++o)
    {
      if (first_read[kid[o]] == NONE) first_read[kid[o]] = k;
      if (cand_sc[kid[o]] != -2 && ksc[o] != -1 && ksc[o] != cand_sc[kid[o]]) bad[kid[o]] = 1;
      if (ksc[o] >= 0)
      {
        if (sc_first_read[ksc[o]] == NONE) sc_first_read[ksc[o]] = k;
        if (sc_reader[ksc[o]] == -1) sc_reader[ksc[o]] = (int)kid[o];
        else if (sc_reader[ksc[o]] != (int)kid[o]) sc_reader[ksc[o]] = -2;
      }
    }
  }
  // CLVs deferred by an earlier call
  for (size_t i = 0; old_deferred && i < nclv; ++i)
  {
    if (!old_deferred[i]) continue;
    const int s = cand_sc[i];
    const bool sc_touched = s >= 0 && (sc_nwrites[s] || sc_first_read[s] != NONE);
    if (nwrites[i] == 0 && first_read[i] == NONE && !sc_touched) continue; // (the list does not see it)
    if (nwrites[i] == 0)
    {
      // read only: from its kept table, if its counts are its own
      const bool ok = !bad[i] && (s < 0 || (sc_nwrites[s] == 0 && (sc_reader[s] == -1 || sc_reader[s] == (int)i)));
      if (ok) out.as_tip[i] = 1;
      else out.materialise.push_back((unsigned int)i);
      continue;
    }
    // overwritten: the deferral ends without the bytes if nothing reads them first and its zero counts go with it
    const unsigned int w = first_write[i];
    const bool dead = (first_read[i] == NONE || first_read[i] > w) &&
                      (s < 0 || (ops[w].parent_scaler == s && sc_first_write[s] == w &&
                                 (sc_first_read[s] == NONE || sc_first_read[s] > w)));
    if (dead) out.dropped.push_back((unsigned int)i);
    else out.materialise.push_back((unsigned int)i);
  }
  // tip-tip ops of this list
  for (unsigned int k = 0; k < count; ++k)
  {
    const pllhip_op_t & op = ops[k];
    const unsigned int p = op.parent_clv;
    const int s = op.parent_scaler;
    if (!true_tip(op.child1_clv) || !true_tip(op.child2_clv) || true_tip(p) || (pinned && pinned[p])) continue;
    if (nwrites[p] != 1 || bad[p] || (first_read[p] != NONE && first_read[p] <= k)) continue;
    // (bad[] of a CLV deferred earlier was judged against its OLD scale buffer: against the new one here)
    if (old_deferred && old_deferred[p])
    {
      bool wrong = false;
      for (unsigned int r = k + 1; r < count && !wrong; ++r)
        wrong = (ops[r].child1_clv == p && ops[r].child1_scaler != -1 && ops[r].child1_scaler != s) ||
                (ops[r].child2_clv == p && ops[r].child2_scaler != -1 && ops[r].child2_scaler != s);
      if (wrong) continue;
    }
    if (s >= 0 && (sc_nwrites[s] != 1 || (sc_reader[s] != -1 && sc_reader[s] != (int)p) ||
                   (sc_first_read[s] != NONE && sc_first_read[s] <= k)))
      continue;
    out.defer[k] = 1;
    out.as_tip[p] = 1;
  }
}

bool pllhip_fused_edge_end_stored(const FusedGeom & geom, const FusedDeferral & dd, unsigned int clv,
                                  bool deferred_before, bool pinned)
{
  if (clv >= geom.nclv || geom.is_tip(clv) || pinned) return false;
  if (!deferred_before) return true;
  return std::find(dd.materialise.begin(), dd.materialise.end(), clv) != dd.materialise.end() ||
         std::find(dd.dropped.begin(), dd.dropped.end(), clv) != dd.dropped.end();
}

// What pllhip_fused_unstored and pllhip_fused_quad_products ask of a walked op alike (partials_fused.hpp): how the list
// treats its parent and its scale buffer, and what the finished plans reload from HBM.
namespace
{
struct UnstoredConditions
{
  static constexpr unsigned int NONE = ~0u;
  const FusedGeom & geom;
  const pllhip_op_t * ops;
  unsigned int count;
  const FusedEdge * edge;
  const unsigned char * pinned;
  // how the list treats every CLV and scale buffer (the cherries' rule: pllhip_fused_deferral)
  std::vector<unsigned int> nwrites, first_read, sc_nwrites, sc_first_read;
  std::vector<int> sc_reader; // the one CLV a scale buffer is read with (-1 nobody, -2 several)
  std::vector<const double *> reloaded; // what some op of the plan copies back from HBM

  UnstoredConditions(const FusedGeom & geom_, const pllhip_op_t * ops_, unsigned int count_,
                     const std::vector<std::vector<FusedOp>> & plans, const FusedEdge * edge_, const unsigned char * pinned_)
    : geom(geom_), ops(ops_), count(count_), edge(edge_), pinned(pinned_), nwrites(geom_.nclv, 0), first_read(geom_.nclv, NONE),
      sc_nwrites(geom_.nsc, 0), sc_first_read(geom_.nsc, NONE), sc_reader(geom_.nsc, -1)
  {
    for (unsigned int k = 0; k < count; ++k)
    {
      const pllhip_op_t & op = ops[k];
      ++nwrites[op.parent_clv];
      if (op.parent_scaler >= 0) ++sc_nwrites[op.parent_scaler];
      const unsigned int kid[2] = {op.child1_clv, op.child2_clv};
      const int ksc[2] = {op.child1_scaler, op.child2_scaler};
      for (int o = 0; o < 2; ++o)
      {
        if (first_read[kid[o]] == NONE) first_read[kid[o]] = k;
        if (ksc[o] < 0) continue;
        if (sc_first_read[ksc[o]] == NONE) sc_first_read[ksc[o]] = k;
        if (sc_reader[ksc[o]] == -1) sc_reader[ksc[o]] = (int)kid[o];
        else if (sc_reader[ksc[o]] != (int)kid[o]) sc_reader[ksc[o]] = -2;
      }
    }
    for (const auto & plan : plans)
      for (const FusedOp & f : plan)
      {
        if ((f.dma_flags & 1) && f.left_hbm) reloaded.push_back(f.left_hbm);
        if ((f.dma_flags & 2) && f.right_hbm) reloaded.push_back(f.right_hbm);
      }
    if (edge)
    {
      if ((edge->op.dma_flags & 1) && edge->op.left_hbm) reloaded.push_back(edge->op.left_hbm);
      if ((edge->op.dma_flags & 2) && edge->op.right_hbm) reloaded.push_back(edge->op.right_hbm);
    }
  }

  // a kind-3 op kept in a slot whose parent nothing but its readers' slots needs
  bool pass(const FusedOp & f) const
  {
    if (f.kind != 3 || f.pslot < 0 || f.list_pos < 0 || (unsigned int)f.list_pos >= count) return false;
    const unsigned int k = (unsigned int)f.list_pos;
    const pllhip_op_t & op = ops[k];
    const unsigned int p = op.parent_clv;
    const int s = op.parent_scaler;
    if (geom.is_tip(p) || (pinned && pinned[p])) return false;
    if (edge && (p == edge->parent_clv || p == edge->child_clv)) return false;
    if (nwrites[p] != 1 || first_read[p] == NONE || first_read[p] <= k) return false;
    bool foreign = false; // read with counts that are not its own
    for (unsigned int r = k + 1; r < count && !foreign; ++r)
      foreign = (ops[r].child1_clv == p && ops[r].child1_scaler != -1 && ops[r].child1_scaler != s) ||
                (ops[r].child2_clv == p && ops[r].child2_scaler != -1 && ops[r].child2_scaler != s);
    if (foreign) return false;
    if (s >= 0 && (sc_nwrites[s] != 1 || (sc_reader[s] != -1 && sc_reader[s] != (int)p) ||
                   (sc_first_read[s] != NONE && sc_first_read[s] <= k)))
      return false;
    return std::find(reloaded.begin(), reloaded.end(), (const double *)f.parent) == reloaded.end();
  }
};
}

// Which gathered-gathered parents of a planned list are left unstored (partials_fused.hpp).
unsigned int pllhip_fused_unstored(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                   std::vector<std::vector<FusedOp>> & plans, const FusedEdge * edge,
                                   const unsigned char * pinned)
{
  const UnstoredConditions rule(geom, ops, count, plans, edge, pinned);
  unsigned int n = 0;
  for (auto & plan : plans)
    for (FusedOp & f : plan)
    {
      f.unstored = 0;
      if (f.prod[0] || f.prod[1]) continue; // (a reader of folded products: its value needs the whole mat-vec)
      if (!rule.pass(f)) continue;
      f.unstored = 1;
      ++n;
    }
  return n;
}

// Which parents over two quads are left unstored (partials_fused.hpp).
unsigned int pllhip_fused_quad_products(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                        std::vector<std::vector<FusedOp>> & plans,
                                        const std::vector<std::vector<unsigned char>> & taken, const FusedEdge * edge,
                                        const unsigned char * pinned)
{
  const UnstoredConditions rule(geom, ops, count, plans, edge, pinned);
  unsigned int n = 0;
  for (size_t sg = 0; sg < plans.size() && sg < taken.size(); ++sg)
    for (size_t pos = 0; pos < plans[sg].size() && 2 * pos + 1 < taken[sg].size(); ++pos)
    {
      FusedOp & f = plans[sg][pos];
      // (read as quads, the reader's value is the product of two gathered table rows: a pair product's shape)
      if (f.unstored || !f.prod[0] || !f.prod[1] || !taken[sg][2 * pos] || !taken[sg][2 * pos + 1]) continue;
      if (!rule.pass(f)) continue;
      f.unstored = 1;
      ++n;
    }
  return n;
}

// Which unstored pair products are folded into their reader (partials_fused.hpp).
unsigned int pllhip_fused_fold(const pllhip_op_t * ops, const int * kinds, unsigned int count,
                               const std::vector<std::vector<FusedOp>> & plans, std::vector<unsigned char> & fold, bool quads)
{
  fold.assign(count, 0);
  // how often each CLV is read in the list, and by whom last: one pass
  unsigned int nclv = 0;
  for (unsigned int r = 0; r < count; ++r)
    nclv = std::max(nclv, std::max(ops[r].parent_clv, std::max(ops[r].child1_clv, ops[r].child2_clv)) + 1u);
  std::vector<unsigned int> reads(nclv, 0);
  std::vector<int> reader(nclv, -1);
  for (unsigned int r = 0; r < count; ++r)
  {
    ++reads[ops[r].child1_clv];
    ++reads[ops[r].child2_clv];
    reader[ops[r].child1_clv] = reader[ops[r].child2_clv] = (int)r;
  }
  unsigned int n = 0;
  for (const auto & plan : plans)
    for (const FusedOp & f : plan)
    {
      if (!f.unstored || f.kind != 3 || f.list_pos < 0 || (unsigned int)f.list_pos >= count) continue;
      // (a quad product has a product on both sides; a pair product on neither)
      if (quads != (f.prod[0] && f.prod[1])) continue;
      const unsigned int k = (unsigned int)f.list_pos, p = ops[k].parent_clv;
      // (pllhip_fused_unstored: written once, read only behind op k)
      if (reads[p] != 1 || reader[p] <= (int)k || kinds[reader[p]] != 0) continue;
      fold[k] = 1;
      ++n;
    }
  // (a list kernel walks at least two ops)
  if (n && count - n < 2)
  {
    fold.assign(count, 0);
    n = 0;
  }
  return n;
}

void pllhip_fused_fold_list(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                            const FusedExtra * extras, const unsigned int * rows4, unsigned int count,
                            const std::vector<unsigned char> & fold, FusedFoldList & out, bool quads)
{
  const unsigned int nrows = quads ? 8u : 4u; // rows an op of the list comes with
  out.where.clear();
  out.ops.clear();
  out.args.clear();
  out.kinds.clear();
  out.extras.clear();
  out.rows8.clear();
  out.prod_op.clear();
  out.as_tip.assign(geom.nclv, 0);
  for (size_t i = 0; geom.as_tip && i < geom.nclv; ++i) out.as_tip[i] = geom.as_tip[i];
  std::vector<int> folded_by(geom.nclv, -1); // per CLV: the folded op that forms it
  for (unsigned int k = 0; k < count; ++k)
    if (fold[k])
    {
      folded_by[ops[k].parent_clv] = (int)k;
      out.as_tip[ops[k].parent_clv] = 1;
    }
  for (unsigned int i = 0; i < count; ++i)
  {
    if (fold[i]) continue;
    const pllhip_op_t & op = ops[i];
    PartialsArgs a = args[i];
    int kind = kinds[i];
    FusedExtra x;
    memset(&x, 0, sizeof(x));
    if (extras && quads) x = extras[i]; // (a folded walk's op keeps its products)
    else if (extras)
    {
      x.g[0] = extras[i].g[0];
      x.g[1] = extras[i].g[1];
    }
    unsigned int rows[8] = {0, 0, 0, 0, 0, 0, 0, 0}, from[2] = {0, 0};
    for (unsigned int t = 0; rows4 && t < nrows; ++t) rows[t] = rows4[nrows * (size_t)i + t];
    const int f1 = kind == 0 ? folded_by[op.child1_clv] : -1, f2 = kind == 0 ? folded_by[op.child2_clv] : -1;
    // side `to` of the reader becomes the product op f forms; sc: the scale buffer the reader passes with it
    auto product = [&](int to, int f, int sc) {
      if (extras && !quads)
      {
        x.g[to] = extras[f].g[0];
        x.g2[to] = extras[f].g[1];
      }
      x.prod[to] = 1 | (ops[f].parent_scaler >= 0 ? 2 : 0) | (sc >= 0 ? 4 : 0) | (quads ? 8 : 0);
      from[to] = (unsigned int)f + 1;
      // (a quad product's factors name quad rows, not tip rows)
      for (int t = 0; rows4 && !quads && t < 4; ++t) rows[4 * to + t] = rows4[4 * (size_t)f + t];
    };
    if (f1 >= 0 && f2 >= 0)
    {
      // both operands are products: no inner operand at all -- gathered-gathered to the planner
      kind = 3;
      product(0, f1, op.child1_scaler);
      product(1, f2, op.child2_scaler);
      a.left = a.right = nullptr;
      a.lscaler = a.rscaler = nullptr;
    }
    else if (f1 >= 0 || f2 >= 0)
    {
      // the product plays the tip of a tip-inner op: "left" (x * y is y * x bit for bit)
      kind = 1;
      product(0, f1 >= 0 ? f1 : f2, f1 >= 0 ? op.child1_scaler : op.child2_scaler);
      if (f1 < 0)
      {
        a.right = args[i].left;
        a.rscaler = args[i].lscaler;
        a.lmat = args[i].rmat;
        a.rmat = args[i].lmat;
      }
      a.left = nullptr;
      a.lscaler = nullptr;
    }
    out.where.push_back(i);
    out.ops.push_back(op);
    out.args.push_back(a);
    out.kinds.push_back(kind);
    out.extras.push_back(x);
    out.rows8.insert(out.rows8.end(), rows, rows + 8);
    out.prod_op.insert(out.prod_op.end(), from, from + 2);
  }
}

int pllhip_fused_plan_segments(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                               const FusedExtra * extra, unsigned int count, const unsigned int * seg_of, unsigned int nsegs,
                               unsigned int nslots, std::vector<std::vector<FusedOp>> & plans, unsigned int * reloads)
{
  plans.assign(nsegs, std::vector<FusedOp>());
  *reloads = 0;
  // (one segment: nothing is copied -- tree search hands over a new list on almost every call)
  if (nsegs == 1) return pllhip_fused_plan(geom, ops, args, kinds, count, nslots, plans[0], reloads, extra);
  for (unsigned int sg = 0; sg < nsegs; ++sg)
  {
    std::vector<pllhip_op_t> sops;
    std::vector<PartialsArgs> sargs;
    std::vector<FusedExtra> sextras;
    std::vector<int> skinds, where;
    for (unsigned int i = 0; i < count; ++i)
      if (seg_of[i] == sg)
      {
        sops.push_back(ops[i]);
        sargs.push_back(args[i]);
        skinds.push_back(kinds[i]);
        if (extra) sextras.push_back(extra[i]);
        where.push_back((int)i);
      }
    unsigned int r = 0;
    const int rc = pllhip_fused_plan(geom, sops.data(), sargs.data(), skinds.data(), (unsigned int)sops.size(), nslots, plans[sg], &r,
                                     extra ? sextras.data() : nullptr);
    if (rc) return rc;
    *reloads += r;
    for (FusedOp & f : plans[sg]) f.list_pos = where[f.list_pos];
  }
  return 0;
}

// Three workgroups per CU (12 waves) hide the per-op latencies better than two, but
// leave one LDS slot less per wave (6 against 7 at 4 rate categories): the 12-wave
// configuration whenever the planner can keep every operand in a slot with it (values
// that give their slot up, and operands written by earlier calls, are copied back from
// HBM by LDS-DMA one op ahead).  A list the planner does not take -- counts that were not
// written together with their CLV -- runs per level.
int pllhip_fused_plan_list(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                           const FusedExtra * extra, unsigned int count, unsigned int max_segments,
                           const unsigned int * slot_counts, unsigned int nslot_counts, FusedEdge * edge,
                           const FusedDeferral & dd, FusedListPlan & out)
{
  std::vector<unsigned int> seg_of;
  unsigned int nsegs = pllhip_fused_segments(geom, ops, count, max_segments, seg_of);
  out.folded = false;
  int rc = 1;
  for (; rc > 0; nsegs = 1) // (segments the planner does not take: once more as one list)
  {
    for (unsigned int t = 0; rc > 0 && t < nslot_counts; ++t)
    {
      out.taken = t;
      out.nslots = slot_counts[t];
      rc = pllhip_fused_plan_segments(geom, ops, args, kinds, extra, count, seg_of.data(), nsegs, out.nslots, out.plans, &out.reloads);
    }
    if (nsegs == 1) break;
  }
  if (rc) return rc;
  // The edge epilogue: one segment only, at the configuration the unfolded plan has just taken (never fewer waves for
  // its sake), both ends ordinary stored CLVs of which the list writes at least one.
  if (edge && out.plans.size() == 1 &&
      pllhip_fused_edge_end_stored(geom, dd, edge->parent_clv, edge->deferred_before[0], edge->pinned[0]) &&
      pllhip_fused_edge_end_stored(geom, dd, edge->child_clv, edge->deferred_before[1], edge->pinned[1]))
  {
    std::vector<FusedOp> with_edge;
    unsigned int reloads = 0;
    if (pllhip_fused_plan(geom, ops, args, kinds, count, out.nslots, with_edge, &reloads, extra, edge) == 0)
    {
      out.plans[0].swap(with_edge);
      out.reloads = reloads;
      out.folded = true;
    }
  }
  return 0;
}

// Plan, unstored, fold, plan once more, unstored (partials_fused.hpp).
int pllhip_fused_plan_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                           const FusedExtra * extras, const unsigned int * rows4, unsigned int count,
                           unsigned int max_segments, const unsigned int * slot_counts, unsigned int nslot_counts,
                           const FusedEdge * edge, const FusedDeferral & dd, const unsigned char * pinned,
                           bool may_unstore, bool may_fold, FusedWalk & out)
{
  out.replanned = false;
  out.nunstored = out.nfolded = out.first_nunstored = 0;
  out.fold.assign(count, 0);
  out.list_ops = ops;
  out.list_rows4 = rows4;
  memset(&out.edge, 0, sizeof(out.edge));
  if (edge) out.edge = *edge;
  FusedEdge * const e = edge ? &out.edge : nullptr;
  const int rc = pllhip_fused_plan_list(geom, ops, args, kinds, extras, count, max_segments, slot_counts, nslot_counts, e, dd, out.plan);
  if (rc || !may_unstore) return rc;
  out.nunstored = pllhip_fused_unstored(geom, ops, count, out.plan.plans, e, pinned);
  if (!out.nunstored || !may_fold || !pllhip_fused_fold(ops, kinds, count, out.plan.plans, out.fold)) return 0;
  pllhip_fused_fold_list(geom, ops, args, kinds, extras, rows4, count, out.fold, out.fl);
  const unsigned int n2 = (unsigned int)out.fl.ops.size();
  FusedGeom geom2 = geom;
  geom2.as_tip = out.fl.as_tip.data();
  FusedListPlan second;
  FusedEdge edge2 = out.edge;
  const bool offer2 = edge && out.plan.plans.size() == 1;
  const int rc2 = n2 < 2 ? 1 : pllhip_fused_plan_list(geom2, out.fl.ops.data(), out.fl.args.data(), out.fl.kinds.data(), out.fl.extras.data(),
                                                      n2, max_segments, slot_counts, nslot_counts, offer2 ? &edge2 : nullptr, dd, second);
  if (rc2)
  {
    out.fold.assign(count, 0);
    return rc2 < 0 ? rc2 : 0;
  }
  out.first_plan = std::move(out.plan);
  out.first_edge = out.edge;
  out.first_nunstored = out.nunstored;
  out.plan = std::move(second);
  out.edge = edge2;
  out.replanned = true;
  for (unsigned int i = 0; i < count; ++i) out.nfolded += out.fold[i];
  out.nunstored = pllhip_fused_unstored(geom2, out.fl.ops.data(), n2, out.plan.plans, e, pinned);
  return 0;
}

// The quad fold: fold, the list without the folded ops, planned once more (partials_fused.hpp).
int pllhip_fused_quad_fold_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * kinds,
                                const FusedExtra * extras, const unsigned int * rows8, unsigned int count,
                                const std::vector<std::vector<FusedOp>> & plans, unsigned int max_segments, unsigned int nslots,
                                const FusedEdge * edge, const FusedDeferral & dd, FusedQuadFold & out)
{
  out.nfolded = pllhip_fused_fold(ops, kinds, count, plans, out.fold, true);
  if (!out.nfolded) return 1;
  pllhip_fused_fold_list(geom, ops, args, kinds, extras, rows8, count, out.fold, out.fl, true);
  const unsigned int n2 = (unsigned int)out.fl.ops.size();
  FusedGeom geom2 = geom;
  geom2.as_tip = out.fl.as_tip.data();
  memset(&out.edge, 0, sizeof(out.edge));
  if (edge) out.edge = *edge;
  const int rc = pllhip_fused_plan_list(geom2, out.fl.ops.data(), out.fl.args.data(), out.fl.kinds.data(), out.fl.extras.data(), n2,
                                        max_segments, &nslots, 1, edge ? &out.edge : nullptr, dd, out.plan);
  if (rc) return rc < 0 ? rc : 1;
  // (the edge pseudo-op stays where the plan before had it)
  if (edge && !out.plan.folded) return 1;
  // what every op was given in the plan before
  std::vector<const FusedOp *> before(count, nullptr);
  for (const auto & plan : plans)
    for (const FusedOp & f : plan)
      if (f.list_pos >= 0 && (unsigned int)f.list_pos < count) before[f.list_pos] = &f;
  std::vector<const double *> reloaded;
  for (const auto & plan : out.plan.plans)
    for (const FusedOp & f : plan)
    {
      if ((f.dma_flags & 1) && f.left_hbm) reloaded.push_back(f.left_hbm);
      if ((f.dma_flags & 2) && f.right_hbm) reloaded.push_back(f.right_hbm);
    }
  if (out.plan.folded)
  {
    if ((out.edge.op.dma_flags & 1) && out.edge.op.left_hbm) reloaded.push_back(out.edge.op.left_hbm);
    if ((out.edge.op.dma_flags & 2) && out.edge.op.right_hbm) reloaded.push_back(out.edge.op.right_hbm);
  }
  for (auto & plan : out.plan.plans)
    for (FusedOp & f : plan)
    {
      const FusedOp * const b = f.list_pos >= 0 && (unsigned int)f.list_pos < n2 ? before[out.fl.where[f.list_pos]] : nullptr;
      if (!b) return 1;
      f.unstored = b->unstored;
      // (pllhip_fused_unstored's conditions on the finished plan: held by the plan before, asked of this one again)
      if (f.unstored && (f.pslot < 0 || std::find(reloaded.begin(), reloaded.end(), (const double *)f.parent) != reloaded.end())) return 1;
      for (int s = 0; s < 2; ++s)
      {
        f.keep[s] = b->keep[s];
        const unsigned int from = out.fl.prod_op[2 * (size_t)f.list_pos + s];
        if (!(f.prod[s] & 8))
        {
          f.pkeep[s][0] = b->pkeep[s][0];
          f.pkeep[s][1] = b->pkeep[s][1];
          continue;
        }
        // the op folded into this side: its two sides, folded products both, are the two quads
        const FusedOp * const q = from ? before[from - 1] : nullptr;
        if (!q || !q->unstored || !q->prod[0] || !q->prod[1]) return 1;
        for (int t = 0; t < 2; ++t)
        {
          f.q[s][t].a = q->g[t];
          f.q[s][t].b = q->g2[t];
          f.q[s][t].mat = t == 0 ? q->lmat : q->rmat;
          f.q[s][t].pkeep[0] = q->pkeep[t][0];
          f.q[s][t].pkeep[1] = q->pkeep[t][1];
          f.qkeep[s][t] = q->keep[t];
        }
      }
    }
  return 0;
}

// ---- the 20-state list (partials_fused.hpp): classes, certificate bounds, the walk

int pllhip_aa_list_classify(const FusedGeom & geom, const pllhip_op_t * ops, const int * kinds, const int * scales,
                            unsigned int count, unsigned int lookups_max, bool tt_inside, AaListClasses & out)
{
  std::vector<unsigned char> clv_touched(geom.nclv, 0), sc_touched(geom.nsc, 0);
  std::vector<int> tt_writer(geom.nclv, -1); // the tip-tip op of this list that wrote each CLV last
  out.cls.assign(count, AA_OP_II);
  out.lk_kids.assign(count, {-1, -1});
  out.lookups = 0;
  out.any_scaler = false;
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_op_t & op = ops[i];
    const int plain = kinds[i];
    if (plain == 2 && (clv_touched[op.parent_clv] || (op.parent_scaler >= 0 && sc_touched[op.parent_scaler]))) return 1;
    out.any_scaler = out.any_scaler || scales[i] != 0;
    out.cls[i] = plain == 2 ? (tt_inside ? AA_OP_TT_LIST : AA_OP_TT_AHEAD) : plain;
    if (out.lookups < lookups_max && plain == 0 && tt_writer[op.child1_clv] >= 0 && tt_writer[op.child2_clv] >= 0)
    {
      out.lk_kids[i] = {tt_writer[op.child1_clv], tt_writer[op.child2_clv]};
      out.cls[i] = AA_OP_LOOKUP;
      ++out.lookups;
    }
    else if (out.lookups < lookups_max && plain == 1)
    {
      const unsigned int inner = geom.is_tip(op.child1_clv) ? op.child2_clv : op.child1_clv;
      if (tt_writer[inner] >= 0)
      {
        out.lk_kids[i] = {-2, tt_writer[inner]};
        out.cls[i] = AA_OP_LOOKUP;
        ++out.lookups;
      }
    }
    tt_writer[op.parent_clv] = plain == 2 ? (int)i : -1;
    clv_touched[op.parent_clv] = clv_touched[op.child1_clv] = clv_touched[op.child2_clv] = 1;
    if (op.parent_scaler >= 0) sc_touched[op.parent_scaler] = 1;
    if (op.child1_scaler >= 0) sc_touched[op.child1_scaler] = 1;
    if (op.child2_scaler >= 0) sc_touched[op.child2_scaler] = 1;
  }
  return 0;
}

void pllhip_aa_list_cert(const FusedGeom & geom, const pllhip_op_t * ops, const int * cls, unsigned int count,
                         const double * incoming, bool ti_mfma, AaListCert & out)
{
  const size_t nclv = geom.nclv, nsc = geom.nsc;
  // a list that overwrites an operand it has read from an earlier call (slot reuse across calls) is not idempotent:
  // it could not be run again after a trip, and keeps to the reference's order
  bool rerunnable = true;
  {
    std::vector<unsigned char> written(nclv, 0), sc_written(nsc, 0), ext_read(nclv, 0), sc_ext_read(nsc, 0);
    for (unsigned int i = 0; i < count && ti_mfma; ++i)
    {
      const pllhip_op_t & op = ops[i];
      for (unsigned int ch : {op.child1_clv, op.child2_clv})
        if (!written[ch]) ext_read[ch] = 1;
      for (int sc : {op.child1_scaler, op.child2_scaler})
        if (sc >= 0 && !sc_written[sc]) sc_ext_read[sc] = 1;
      if (ext_read[op.parent_clv] || (op.parent_scaler >= 0 && sc_ext_read[op.parent_scaler])) rerunnable = false;
      written[op.parent_clv] = 1;
      if (op.parent_scaler >= 0) sc_written[op.parent_scaler] = 1;
    }
  }
  out.list_ti_mfma = ti_mfma && rerunnable;
  out.op_inexact.assign(count, 0);
  out.out_marks.clear();
  std::vector<double> err(nclv, 0.0);
  std::vector<unsigned char> local(nclv, 0);
  bool any_ti = false;
  double worst = 0.0;
  for (int attempt = 0; attempt < 2; ++attempt)
  {
    // (first with the tip-inner mat-vecs on the matrix cores; if the bounds then outgrow every window -- operands
    // that earlier calls left with large bounds -- once more with every op in the reference's order)
    std::fill(local.begin(), local.end(), 0);
    out.ext_marks.clear();
    any_ti = false;
    worst = 0.0;
    for (unsigned int i = 0; i < count; ++i)
    {
      const pllhip_op_t & op = ops[i];
      const bool source = cls[i] == AA_OP_TI && out.list_ti_mfma;
      any_ti = any_ti || source;
      double in = 0.0;
      for (unsigned int ch : {op.child1_clv, op.child2_clv})
      {
        if (geom.is_tip(ch)) continue;
        if (!local[ch])
        {
          // an operand from an earlier call: the plan holds for THIS bound of it
          const double m = incoming ? incoming[ch] : 0.0;
          bool seen = false;
          for (const auto & e : out.ext_marks) seen = seen || e.first == ch;
          if (!seen) out.ext_marks.push_back({ch, m});
          in += m;
        }
        else in += err[ch];
      }
      const double bound = (source || in > 0.0) ? in + PLLHIP_CERT_OP_ERR : 0.0;
      err[op.parent_clv] = bound;
      local[op.parent_clv] = 1;
      out.op_inexact[i] = bound > 0.0 && op.parent_scaler >= 0;
      if (out.op_inexact[i] && bound > worst) worst = bound;
    }
    if (!(out.list_ti_mfma && 8.0 * worst > PLLHIP_CERT_WINDOW_MAX)) break;
    out.list_ti_mfma = false;
  }
  for (unsigned int i = 0; i < nclv; ++i)
    if (local[i]) out.out_marks.push_back({i, err[i]});
  out.cert_kind = !(worst > 0.0) ? 0 : (any_ti ? 1 : 2);
  out.too_wide = 8.0 * worst > PLLHIP_CERT_WINDOW_MAX;
  out.window = std::min(std::max(8.0 * worst, PLLHIP_CERT_WINDOW_MIN), PLLHIP_CERT_WINDOW_MAX);
}

int pllhip_aa_list_walk(const FusedGeom & geom, const pllhip_op_t * ops, const PartialsArgs * args, const int * cls,
                        const int * scales, unsigned int count, unsigned int max_segments, unsigned int nslots,
                        AaListWalk & out)
{
  std::vector<pllhip_op_t> rops;
  std::vector<PartialsArgs> rargs;
  std::vector<int> rkinds;
  out.ahead.clear();
  out.orig.clear();
  out.plan.clear();
  out.seg_first.clear();
  out.seg_n.clear();
  out.sync_left.clear();
  out.reloads = 0;
  for (int pass = 0; pass < 2; ++pass) // (tip-tip ops grouped by mode: without a scale buffer first)
    for (unsigned int i = 0; i < count; ++i)
      if (cls[i] == AA_OP_TT_AHEAD && (scales[i] != 0) == (pass == 1)) out.ahead.push_back(i);
  for (unsigned int i = 0; i < count; ++i)
    if (cls[i] != AA_OP_TT_AHEAD)
    {
      rops.push_back(ops[i]);
      rargs.push_back(args[i]);
      rkinds.push_back(pllhip_aa_walk_kind(cls[i]));
      out.orig.push_back((int)i);
    }
  const unsigned int n = (unsigned int)rops.size();
  if (n == 0) return 1; // nothing but tip-tip ops
  std::vector<unsigned int> seg_of;
  out.nsegs = pllhip_fused_segments(geom, rops.data(), n, max_segments, seg_of);
  std::vector<std::vector<FusedOp>> seg_plans;
  const int rc = pllhip_fused_plan_segments(geom, rops.data(), rargs.data(), rkinds.data(), nullptr, n, seg_of.data(), out.nsegs,
                                            nslots, seg_plans, &out.reloads);
  if (rc) return rc;
  for (unsigned int sg = 0; sg < out.nsegs; ++sg)
  {
    out.seg_first.push_back((unsigned int)out.plan.size());
    out.seg_n.push_back((unsigned int)seg_plans[sg].size());
    if (sg == 0) out.plan.swap(seg_plans[0]); // (one segment: no copy)
    else out.plan.insert(out.plan.end(), seg_plans[sg].begin(), seg_plans[sg].end());
  }
  out.sync_left.assign(n, 0);
  for (unsigned int sg = 0; sg < out.nsegs; ++sg)
  {
    const FusedOp * f = out.plan.data() + out.seg_first[sg];
    const unsigned int m = out.seg_n[sg];
    for (unsigned int pos = 0; pos < m; ++pos)
      out.sync_left[out.seg_first[sg] + pos] = f[pos].kind == 0 && f[(pos + m - 1) % m].kind == 2;
  }
  return 0;
}

void pllhip_aa_list_kinds_of(const int * cls, unsigned int count, bool list_ti_mfma, unsigned int reloads,
                             unsigned int * out8)
{
  unsigned int n[5] = {0, 0, 0, 0, 0};
  for (unsigned int i = 0; i < count; ++i) ++n[cls[i]];
  const unsigned int v[8] = {count, n[AA_OP_TT_AHEAD], n[AA_OP_TT_LIST], n[AA_OP_LOOKUP], n[AA_OP_II],
                             list_ti_mfma ? n[AA_OP_TI] : 0u, list_ti_mfma ? 0u : n[AA_OP_TI], reloads};
  for (int t = 0; t < 8; ++t) out8[t] = v[t];
}

// ---- the planner without a device (tests, tools): fake addresses, the same code

static int dry_ops_in_range(const char * who, const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count)
{
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_op_t & op = ops[i];
    if (op.parent_clv >= geom.nclv || op.child1_clv >= geom.nclv || op.child2_clv >= geom.nclv ||
        op.parent_scaler >= (int)geom.nsc || op.child1_scaler >= (int)geom.nsc || op.child2_scaler >= (int)geom.nsc)
    {
      pllhip_set_error("%s: index out of range in op %u", who, i);
      return -1;
    }
  }
  return 0;
}
// (distinct fake addresses per CLV and per scale buffer: the reload plan compares them)
static const double * dry_clv(unsigned int idx) { return reinterpret_cast<const double *>((uintptr_t)4096 * (idx + 1)); }
static unsigned int * dry_scaler(int idx) { return idx >= 0 ? reinterpret_cast<unsigned int *>((uintptr_t)4096 * (idx + 1)) : nullptr; }

// What resolve_op (partials.hip) and the deferral make of an op, as far as the planner looks: its kind, the inner
// operands' and the counts' addresses.  operands[2] (may be nullptr): 0 a slot, 1 a tip, 2 a deferred cherry.
static void dry_resolve(const FusedGeom & geom, const pllhip_op_t & op, PartialsArgs & a, int & kind, int * operands)
{
  const bool t1 = geom.is_tip(op.child1_clv), t2 = geom.is_tip(op.child2_clv);
  const bool tip1 = geom.pattern_tip && op.child1_clv < geom.tips, tip2 = geom.pattern_tip && op.child2_clv < geom.tips;
  memset(&a, 0, sizeof(PartialsArgs));
  kind = (tip1 && tip2) ? 2 : (t1 && t2) ? 3 : (t1 || t2) ? 1 : 0;
  a.pscaler = dry_scaler(op.parent_scaler);
  a.parent = const_cast<double *>(dry_clv(op.parent_clv));
  if (kind == 0)
  {
    a.left = dry_clv(op.child1_clv);
    a.right = dry_clv(op.child2_clv);
    a.lscaler = dry_scaler(op.child1_scaler);
    a.rscaler = dry_scaler(op.child2_scaler);
  }
  else if (kind == 1)
  {
    a.right = dry_clv(t1 ? op.child2_clv : op.child1_clv);
    a.rscaler = dry_scaler(t1 ? op.child2_scaler : op.child1_scaler);
  }
  if (operands)
  {
    operands[0] = tip1 ? 1 : t1 ? 2 : 0;
    operands[1] = tip2 ? 1 : t2 ? 2 : 0;
  }
}
static void dry_slots_out(const FusedOp & f, int * six)
{
  const int v[6] = {f.lslot, f.rslot, f.pslot, f.lsc_slot, f.rsc_slot, f.dma_flags};
  for (int t = 0; t < 6; ++t) six[t] = v[t];
}

// (pllhip_fused_plan_dry_quad_products) the final walk as the launch sees it: the plans, the list they were made of --
// the caller's without the deferred and the folded ops --, each of its ops' place in the caller's list, the gathered CLVs
struct DryFinal
{
  std::vector<std::vector<FusedOp>> plans;
  std::vector<pllhip_op_t> ops;
  std::vector<unsigned int> to_list;
  std::vector<unsigned char> as_tip;
  bool has_edge = false;
  FusedEdge edge;
  // (pllhip_fused_plan_dry_quad_fold) what the quad fold plans that list with once more
  std::vector<PartialsArgs> args;
  std::vector<int> kinds;
  std::vector<unsigned int> rows8;
  std::vector<FusedExtra> extras;
  FusedDeferral dd;
  unsigned int nslots = 0;
  bool edge_folded = false;
};

// The planner with deferred cherries, without a device (tests/test_host_deferred_plan.py).  old_deferred / old_scaler /
// pinned: per CLV index, may be NULL (pllhip_fused_deferral).  Out: *nkept kept ops in walk order as positions in
// the caller's list (order_out), six numbers per kept op as pllhip_fused_plan_dry gives them (slots_out), two operand
// kinds per kept op (operands_out: 0 a slot, 1 a tip, 2 a deferred cherry), per list op whether it is deferred
// (deferred_out), and the CLVs deferred earlier that the list has materialised first / ends the deferral of
// (materialise_out, dropped_out: at most clv indices each, counts in *nmaterialise, *ndropped).
// Returns 0, 1 if the kernel does not take the list, < 0 on error.
// (edge4 not null: pllhip_fused_plan_dry_edge -- {parent_clv, parent_scaler, child_clv, child_scaler}; `nslots` is then
// not used: the slot counts are those of 12 and of 8 waves per CU at `rate_cats` categories; final_out not null: the
// final walk as well, DryFinal above)
static int plan_dry_deferred(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                             int pattern_tip, const pllhip_op_t * ops, unsigned int count, unsigned int nslots,
                             const unsigned char * old_deferred, const int * old_scaler,
                             const unsigned char * pinned, unsigned int * nkept, unsigned int * order_out,
                             int * slots_out, int * operands_out, unsigned char * deferred_out,
                             unsigned int * reloads_out, unsigned int * materialise_out,
                             unsigned int * nmaterialise, unsigned int * dropped_out, unsigned int * ndropped,
                             const int * edge4, unsigned int rate_cats, int * edge_out,
                             unsigned char * unstored_out = nullptr, unsigned char * folded_out = nullptr,
                             unsigned int * gathers_out = nullptr, unsigned int * batch_out = nullptr,
                             unsigned int * nbatches_out = nullptr, int * kinds_out = nullptr, DryFinal * final_out = nullptr)
{
  FusedGeom geom = {(size_t)tips + clv_buffers, scale_buffers, tips, pattern_tip != 0};
  if (dry_ops_in_range("pllhip_fused_plan_dry_deferred", geom, ops, count)) return -1;
  for (unsigned int i = 0; unstored_out && i < count; ++i) unstored_out[i] = 0;
  if (edge4 && (edge4[0] < 0 || (size_t)edge4[0] >= geom.nclv || edge4[2] < 0 || (size_t)edge4[2] >= geom.nclv ||
                edge4[1] >= (int)scale_buffers || edge4[3] >= (int)scale_buffers ||
                !(rate_cats == 1 || rate_cats == 2 || rate_cats == 4)))
  {
    pllhip_set_error("pllhip_fused_plan_dry_edge: bad edge or rate_cats");
    return -1;
  }
  FusedDeferral d;
  pllhip_fused_deferral(geom, ops, count, old_deferred, old_scaler, pinned, d);
  std::vector<pllhip_op_t> kept;
  std::vector<unsigned int> where;
  for (unsigned int i = 0; i < count; ++i)
  {
    if (deferred_out) deferred_out[i] = d.defer[i];
    if (!d.defer[i])
    {
      kept.push_back(ops[i]);
      where.push_back(i);
    }
  }
  if (nmaterialise) *nmaterialise = (unsigned int)d.materialise.size();
  if (ndropped) *ndropped = (unsigned int)d.dropped.size();
  for (size_t t = 0; materialise_out && t < d.materialise.size(); ++t) materialise_out[t] = d.materialise[t];
  for (size_t t = 0; dropped_out && t < d.dropped.size(); ++t) dropped_out[t] = d.dropped[t];
  // (what is materialised first is an ordinary buffer to the list)
  for (unsigned int i : d.materialise) d.as_tip[i] = 0;
  geom.as_tip = d.as_tip.data();
  unsigned int n = (unsigned int)kept.size();
  if (nkept) *nkept = n;
  for (unsigned int i = 0; folded_out && i < count; ++i) folded_out[i] = 0;
  std::vector<PartialsArgs> args(n);
  std::vector<int> kinds(n), opnd(2 * (size_t)n);
  for (unsigned int i = 0; i < n; ++i) dry_resolve(geom, kept[i], args[i], kinds[i], &opnd[2 * i]);
  for (unsigned int i = 0; operands_out && i < 2 * n; ++i) operands_out[i] = opnd[i];
  if (reloads_out) *reloads_out = 0;
  for (int t = 0; edge_out && t < 8; ++t) edge_out[t] = t >= 1 && t <= 4 ? -1 : 0;
  if (!n) return 0;
  // one segment; with an edge the slot counts of a partition with per-site or no scale buffers
  // (pllhip_fused_plan_dry_unstored with nslots 0: the same two)
  const bool derived = edge4 || (!nslots && rate_cats);
  const unsigned int slot_counts[2] = {derived ? pllhip_fused_slots_for(rate_cats, false, 3) : nslots,
                                       derived ? pllhip_fused_slots_for(rate_cats, false, 2) : 0u};
  FusedEdge e;
  memset(&e, 0, sizeof(e));
  if (edge4)
  {
    e.parent_clv = (unsigned int)edge4[0];
    e.parent_scaler = edge4[1];
    e.child_clv = (unsigned int)edge4[2];
    e.child_scaler = edge4[3];
    e.parent = dry_clv(e.parent_clv);
    e.child = dry_clv(e.child_clv);
    e.pscaler = dry_scaler(e.parent_scaler);
    e.cscaler = dry_scaler(e.child_scaler);
    // (an end deferred by an earlier call that the list does not see is not in HBM)
    const unsigned int ends[2] = {e.parent_clv, e.child_clv};
    for (int t = 0; t < 2; ++t)
    {
      e.deferred_before[t] = old_deferred && old_deferred[ends[t]];
      e.pinned[t] = pinned && pinned[ends[t]];
    }
  }
  // (pllhip_fused_plan_dry_rows) the tip rows of every kept op's gathered factors, tip index + 1, as the live path
  // hands them over: a gathered child's one or two rows -- a tip's own, a cherry's two tips (deferred by this list) --,
  // the first gathered child's at [0, 1], the second's at [2, 3]; a tip-tip op's two tips at [0, 1]
  std::vector<unsigned int> rows4;
  if (gathers_out)
  {
    std::vector<int> deferring_op(geom.nclv, -1);
    for (unsigned int i = 0; i < count; ++i)
      if (d.defer[i]) deferring_op[ops[i].parent_clv] = (int)i;
    rows4.assign(4 * (size_t)n, 0u);
    for (unsigned int i = 0; i < n; ++i)
    {
      const unsigned int kid[2] = {kept[i].child1_clv, kept[i].child2_clv};
      unsigned int at = 0;
      for (int t = 0; t < 2 && kinds[i] != 0; ++t)
      {
        if (!geom.is_tip(kid[t])) continue;
        unsigned int * r = &rows4[4 * (size_t)i + (kinds[i] == 2 ? 0 : 2 * at)];
        if (geom.pattern_tip && kid[t] < geom.tips) r[kinds[i] == 2 ? t : 0] = kid[t] + 1;
        else if (deferring_op[kid[t]] >= 0)
        {
          r[0] = ops[deferring_op[kid[t]]].child1_clv + 1;
          r[1] = ops[deferring_op[kid[t]]].child2_clv + 1;
        }
        ++at;
      }
    }
  }
  // the live path's steps: pllhip_fused_plan_walk
  FusedWalk w;
  const int rc = pllhip_fused_plan_walk(geom, kept.data(), args.data(), kinds.data(), nullptr, gathers_out ? rows4.data() : nullptr, n, 1, slot_counts, derived ? 2u : 1u,
                                        edge4 ? &e : nullptr, d, pinned, unstored_out != nullptr, folded_out != nullptr, w);
  if (rc) return rc;
  const std::vector<FusedOp> & plan = w.plan.plans[0];
  n = (unsigned int)plan.size();
  if (nkept) *nkept = n;
  for (unsigned int k = 0; folded_out && k < (unsigned int)kept.size(); ++k)
    if (w.fold[k]) folded_out[where[k]] = 1;
  if (edge4)
  {
    const int wgs = 3 - (int)w.plan.taken; // workgroups per CU of the slot count taken
    edge_out[6] = wgs;
    if (w.plan.folded)
    {
      const FusedOp & eo = w.edge.op;
      const int v[8] = {1, eo.lslot, eo.rslot, eo.lsc_slot, eo.rsc_slot, eo.dma_flags, wgs, wgs};
      for (int t = 0; t < 8; ++t) edge_out[t] = v[t];
    }
  }
  for (unsigned int pos = 0; pos < n; ++pos)
  {
    const FusedOp & f = plan[pos];
    const unsigned int o = w.pos_in_list(f);
    if (unstored_out && f.unstored) unstored_out[where[o]] = 1;
    if (order_out) order_out[pos] = where[o];
    if (operands_out)
    {
      // (3: a product folded into that side)
      const unsigned int kid[2] = {kept[o].child1_clv, kept[o].child2_clv};
      for (int t = 0; t < 2; ++t)
        operands_out[2 * pos + t] = w.replanned && w.fl.as_tip[kid[t]] && !geom.is_tip(kid[t]) ? 3 : opnd[2 * o + t];
    }
    if (slots_out) dry_slots_out(f, slots_out + (size_t)pos * 6);
    // (pllhip_fused_plan_dry_quads: the kind the kernel runs and the folded products on its two sides)
    if (kinds_out)
    {
      kinds_out[3 * pos] = f.kind;
      kinds_out[3 * pos + 1] = f.prod[0];
      kinds_out[3 * pos + 2] = f.prod[1];
    }
  }
  if (reloads_out) *reloads_out = w.plan.reloads;
  if (final_out)
  {
    final_out->plans = w.plan.plans;
    final_out->ops = w.replanned ? w.fl.ops : kept;
    final_out->to_list.resize(final_out->ops.size());
    for (unsigned int i = 0; i < final_out->ops.size(); ++i) final_out->to_list[i] = where[w.replanned ? w.fl.where[i] : i];
    final_out->as_tip = w.replanned ? w.fl.as_tip : d.as_tip;
    final_out->has_edge = edge4 != nullptr;
    final_out->edge = w.edge;
    final_out->args = w.replanned ? w.fl.args : args;
    final_out->kinds = w.replanned ? w.fl.kinds : kinds;
    if (w.replanned) final_out->rows8 = w.fl.rows8;
    if (w.replanned) final_out->extras = w.fl.extras; // (no operands without a device; the products of each op)
    final_out->dd = d;
    final_out->nslots = w.plan.nslots;
    final_out->edge_folded = w.plan.folded;
  }
  if (gathers_out)
  {
    // What each walked op gathers, in the order the kernel does (partials_fused.hip: fused_seg_gathers): a reader of
    // folded products the two factors of the product on its left, then of the one on its right; else the op's own one
    // or two.  Every factor names ONE row (pllhip_fused_gather_rows / _bits), dealt to batches by the one rule.
    std::vector<unsigned int> ntips(n, 0u);
    for (unsigned int pos = 0; pos < n; ++pos)
    {
      const FusedOp & f = plan[pos];
      unsigned int r8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (w.replanned) memcpy(r8, &w.fl.rows8[8 * (size_t)f.list_pos], sizeof(r8));
      else memcpy(r8, &rows4[4 * (size_t)f.list_pos], 4 * sizeof(unsigned int));
      unsigned int * g = gathers_out + 12 * (size_t)pos;
      for (int k = 0; k < 4; ++k)
      {
        g[3 * k] = r8[2 * k];
        g[3 * k + 1] = r8[2 * k + 1];
        g[3 * k + 2] = 0;
        ntips[pos] |= pllhip_fused_gather_rows(r8[2 * k] != 0, r8[2 * k + 1] != 0) << (2 * k);
      }
    }
    const unsigned int ts = PLLHIP_FUSED_J * (64 / (2 * (rate_cats ? rate_cats : 4u)));
    std::vector<unsigned int> ch[4], batch(n, 0u);
    for (int k = 0; k < 4; ++k) ch[k].assign(n, 0u);
    unsigned int * const chars_out[4] = {ch[0].data(), ch[1].data(), ch[2].data(), ch[3].data()};
    const unsigned int nb = pllhip_fused_char_batches8(ntips.data(), n, ts >= 16 ? ts / 16 : 1, chars_out, batch.data());
    for (unsigned int pos = 0; pos < n; ++pos)
    {
      unsigned int * g = gathers_out + 12 * (size_t)pos;
      for (int k = 0; k < 4; ++k) g[3 * k + 2] = ch[k][pos] | pllhip_fused_gather_bits(g[3 * k] != 0, g[3 * k + 1] != 0);
      if (batch_out) batch_out[pos] = batch[pos];
    }
    if (nbatches_out) *nbatches_out = nb;
  }
  return 0;
}

// The rows the kernel's gathers name, without a device or a pool (tests/test_host_pair_rows.py): the final walk of
// pllhip_fused_plan_dry_folded, and per walked op gathers_out[12] = four gathers x {first tip + 1, second tip + 1 (both
// set: the pair row of that ordered pair; one: that tip's own row; neither: no gather), the record's chars word:
// PLLHIP_FUSED_CH_LPOS the row's first lane in its batch, CH_LTIP, CH_SHIFT4, CH_NIBBLE}; batch_out per walked op,
// *nbatches_out in all.
extern "C" int pllhip_fused_plan_dry_rows(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                          int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops, unsigned int count,
                                          unsigned int nslots, unsigned int * nkept, unsigned int * order_out,
                                          unsigned char * deferred_out, unsigned char * folded_out,
                                          unsigned int * gathers_out, unsigned int * batch_out, unsigned int * nbatches_out)
{
  if (!(rate_cats == 1 || rate_cats == 2 || rate_cats == 4) || !folded_out || !gathers_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_rows: rate_cats of an instance that defers, folded_out and gathers_out");
    return -1;
  }
  int edge_out[8];
  std::vector<unsigned char> unstored(count, 0);
  return plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, nslots, nullptr, nullptr, nullptr, nkept,
                           order_out, nullptr, nullptr, deferred_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, rate_cats, edge_out, unstored.data(), folded_out, gathers_out, batch_out, nbatches_out);
}

// Which folded products are read as quads (quad_rows.hip; tests/test_host_quad_rows.py): the final walk of
// pllhip_fused_plan_dry_rows, then the rule the live path applies (pllhip_fused_quad_decide) -- to a partition of `sites`
// sites with quad rows `quads_on` at `min_sites_per_class`.  What the live path finds on the device or in the context is
// handed in per op of the caller's list, read where the op is a folded product: classes[i] the class count of its quad
// row (0: beyond the cap), bounds[i] the lower bound the host can prove for its table (NULL or <= 0: none).
// ops_out[3 pos ..]: walked op pos's kind, its gathers and how many of them are wide.  quads_out[i]: -1 where op i is no
// folded product, else the rule's answer (0: read as a quad; else the reason, pllhip.h).  counts_out[2]: quads taken,
// and refused (of the products over two cherries, as pllhip_quad_row_stats counts them).
// (products_out / bytes_out: pllhip_fused_plan_dry_quad_products, below)
static int plan_dry_quads(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                          int pattern_tip, unsigned int rate_cats, int rate_scalers, const pllhip_op_t * ops,
                          unsigned int count, unsigned int nslots, const unsigned char * pinned, const int * edge4,
                          unsigned int sites, int quads_on, unsigned int min_sites_per_class,
                          const unsigned int * classes, const double * bounds, unsigned int * nkept,
                          unsigned int * order_out, unsigned char * folded_out, int * ops_out, int * quads_out,
                          unsigned int * counts_out, unsigned char * products_out, unsigned int * bytes_out,
                          int fold_on = 0, unsigned char * qfolded_out = nullptr, unsigned int * walked_out = nullptr)
{
  if (!(rate_cats == 1 || rate_cats == 2 || rate_cats == 4) || !classes || !nkept || !order_out || !folded_out || !ops_out || !quads_out ||
      !counts_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_quads: rate_cats of an instance that defers, and every output");
    return -1;
  }
  int edge_out[8];
  DryFinal fin;
  std::vector<unsigned char> unstored(count, 0), deferred(count, 0);
  std::vector<unsigned int> gathers(12 * (size_t)count + 12, 0u);
  std::vector<int> kinds(3 * (size_t)count + 3, 0);
  const int rc = plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, nslots, nullptr, nullptr, pinned, nkept,
                                   order_out, nullptr, nullptr, deferred.data(), nullptr, nullptr, nullptr, nullptr, nullptr, edge4,
                                   rate_cats, edge_out, unstored.data(), folded_out, gathers.data(), nullptr, nullptr, kinds.data(),
                                   products_out ? &fin : nullptr);
  if (rc) return rc;
  for (unsigned int i = 0; i < count; ++i) quads_out[i] = -1;
  counts_out[0] = counts_out[1] = 0;
  // the tips under a child of a folded op: itself, or the two of the cherry this list defers
  auto tips_of = [&](unsigned int clv, unsigned int (&t)[2]) {
    t[0] = t[1] = 0;
    if (clv < tips) { t[0] = clv + 1; return; }
    for (unsigned int i = 0; i < count; ++i)
      if (deferred[i] && ops[i].parent_clv == clv) { t[0] = ops[i].child1_clv + 1; t[1] = ops[i].child2_clv + 1; }
  };
  std::vector<FusedQuadCand> cands;
  std::vector<unsigned int> op_of;
  for (unsigned int pos = 0; pos < *nkept; ++pos)
  {
    const pllhip_op_t & reader = ops[order_out[pos]];
    const unsigned int * g = &gathers[12 * (size_t)pos];
    for (int s = 0; s < 2; ++s)
    {
      const int prod = kinds[3 * pos + 1 + s];
      if (!prod) continue;
      // the folded op on this side: the child of the reader whose factors' rows the side's two gathers name
      unsigned int found = count;
      for (unsigned int j = 0; j < count && found == count; ++j)
      {
        if (!folded_out[j] || (ops[j].parent_clv != reader.child1_clv && ops[j].parent_clv != reader.child2_clv)) continue;
        unsigned int a[2], b[2];
        tips_of(ops[j].child1_clv, a);
        tips_of(ops[j].child2_clv, b);
        const unsigned int * ga = g + 6 * s, * gb = g + 6 * s + 3;
        auto same = [](const unsigned int (&t)[2], const unsigned int * r) {
          return (t[0] == r[0] && t[1] == r[1]) || (t[1] == 0 && r[0] == 0 && t[0] == r[1]);
        };
        if ((same(a, ga) && same(b, gb)) || (same(b, ga) && same(a, gb))) found = j;
      }
      if (found == count)
      {
        pllhip_set_error("pllhip_fused_plan_dry_quads: op %u's folded operand is not in the list", order_out[pos]);
        return -1;
      }
      const bool cherries = g[6 * s] && g[6 * s + 1] && g[6 * s + 3] && g[6 * s + 4];
      cands.push_back(FusedQuadCand{0u, pos, s, kinds[3 * pos + 1] && kinds[3 * pos + 2], cherries, classes[found], (prod & 2) != 0,
                                    bounds ? bounds[found] : 0.0, 0});
      op_of.push_back(found);
    }
  }
  const bool instance = quads_on && pattern_tip && rate_cats <= 4 && !rate_scalers;
  counts_out[0] = pllhip_fused_quad_decide(cands.data(), cands.size(), instance, sites, min_sites_per_class ? min_sites_per_class : 64u);
  std::vector<unsigned char> taken(2 * (size_t)*nkept + 2, 0);
  for (size_t i = 0; i < cands.size(); ++i)
  {
    quads_out[op_of[i]] = cands[i].reason;
    taken[2 * (size_t)cands[i].pos + cands[i].side] = cands[i].reason == FUSED_QUAD_TAKEN;
    counts_out[1] += cands[i].cherries && cands[i].reason != FUSED_QUAD_TAKEN;
  }
  for (unsigned int pos = 0; pos < *nkept; ++pos)
  {
    const unsigned int * g = &gathers[12 * (size_t)pos];
    int ng = 0, wide = 0;
    if (taken[2 * pos] || taken[2 * pos + 1])
      // (a reader of quads: one wide gather per product -- both, or the only one)
      ng = wide = (kinds[3 * pos + 1] != 0) + (kinds[3 * pos + 2] != 0);
    else
      for (int k = 0; k < 4; ++k) ng += g[3 * k] || g[3 * k + 1];
    ops_out[3 * pos] = kinds[3 * pos];
    ops_out[3 * pos + 1] = ng;
    ops_out[3 * pos + 2] = wide;
  }
  if (!products_out) return 0;
  // the launch's step behind the quads' (partials_fused.hip): pllhip_fused_quad_products on the final walk
  for (unsigned int i = 0; i < count; ++i) products_out[i] = 0;
  FusedGeom geom = {(size_t)tips + clv_buffers, scale_buffers, tips, pattern_tip != 0, fin.as_tip.data()};
  const std::vector<std::vector<unsigned char>> marks(1, taken);
  const bool any = pllhip_fused_quad_products(geom, fin.ops.data(), (unsigned int)fin.ops.size(), fin.plans, marks,
                                              fin.has_edge ? &fin.edge : nullptr, pinned) != 0;
  // (pllhip_fused_plan_dry_quad_fold) ... and the quad fold behind it: the plan it makes stands in for the walk's
  for (unsigned int i = 0; qfolded_out && i < count; ++i) qfolded_out[i] = 0;
  FusedQuadFold qf;
  if (any && fold_on && !fin.rows8.empty() &&
      pllhip_fused_quad_fold_walk(geom, fin.ops.data(), fin.args.data(), fin.kinds.data(), fin.extras.data(), fin.rows8.data(),
                                  (unsigned int)fin.ops.size(), fin.plans, 1, fin.nslots, fin.edge_folded ? &fin.edge : nullptr, fin.dd, qf) == 0)
  {
    for (unsigned int i = 0; i < fin.ops.size(); ++i)
      if (qf.fold[i])
      {
        products_out[fin.to_list[i]] = 1;
        if (qfolded_out) qfolded_out[fin.to_list[i]] = 1;
      }
    std::vector<unsigned int> to_list(qf.fl.ops.size());
    for (unsigned int i = 0; i < to_list.size(); ++i) to_list[i] = fin.to_list[qf.fl.where[i]];
    fin.to_list.swap(to_list);
    fin.plans = qf.plan.plans;
  }
  if (walked_out) *walked_out = (unsigned int)fin.plans[0].size();
  // ... and the plan's bytes per site, as DESIGN.md 2.0 counts them: one write per entry of a stored CLV and per count,
  // one read per character of the tips under the list
  unsigned int bytes = 0;
  for (const FusedOp & f : fin.plans[0])
  {
    if (f.list_pos < 0 || (size_t)f.list_pos >= fin.to_list.size()) continue;
    if (f.unstored && f.prod[0] && f.prod[1]) products_out[fin.to_list[f.list_pos]] = 1;
    bytes += (f.unstored ? 0u : 4u * rate_cats * 8u) + (f.pscaler ? (rate_scalers ? 4u * rate_cats : 4u) : 0u);
  }
  std::vector<unsigned char> read(tips, 0);
  for (unsigned int i = 0; pattern_tip && i < count; ++i)
  {
    if (ops[i].child1_clv < tips) read[ops[i].child1_clv] = 1;
    if (ops[i].child2_clv < tips) read[ops[i].child2_clv] = 1;
  }
  for (unsigned int t = 0; t < tips; ++t) bytes += read[t];
  if (bytes_out) *bytes_out = bytes;
  return 0;
}

extern "C" int pllhip_fused_plan_dry_quads(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                           int pattern_tip, unsigned int rate_cats, int rate_scalers, const pllhip_op_t * ops,
                                           unsigned int count, unsigned int nslots, const unsigned char * pinned, const int * edge4,
                                           unsigned int sites, int quads_on, unsigned int min_sites_per_class,
                                           const unsigned int * classes, const double * bounds, unsigned int * nkept,
                                           unsigned int * order_out, unsigned char * folded_out, int * ops_out, int * quads_out,
                                           unsigned int * counts_out)
{
  return plan_dry_quads(tips, clv_buffers, scale_buffers, pattern_tip, rate_cats, rate_scalers, ops, count, nslots, pinned, edge4, sites,
                        quads_on, min_sites_per_class, classes, bounds, nkept, order_out, folded_out, ops_out, quads_out, counts_out,
                        nullptr, nullptr);
}

// Quad products without a device (deferred.hip; tests/test_host_quad_products.py): pllhip_fused_plan_dry_quads, then the
// rule the launch applies behind the quads' (pllhip_fused_quad_products).  products_out[i] = 1: op i of the caller's
// list is walked over two taken quads and its parent is not stored.  *bytes_out: the plan's bytes per site -- one write
// per entry of every stored CLV of the walk and per count, one read per character of the tips under the list.
extern "C" int pllhip_fused_plan_dry_quad_products(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                   int pattern_tip, unsigned int rate_cats, int rate_scalers, const pllhip_op_t * ops,
                                                   unsigned int count, unsigned int nslots, const unsigned char * pinned,
                                                   const int * edge4, unsigned int sites, int quads_on,
                                                   unsigned int min_sites_per_class, const unsigned int * classes,
                                                   const double * bounds, unsigned int * nkept, unsigned int * order_out,
                                                   unsigned char * folded_out, int * ops_out, int * quads_out,
                                                   unsigned int * counts_out, unsigned char * products_out, unsigned int * bytes_out)
{
  if (!products_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_quad_products: products_out");
    return -1;
  }
  return plan_dry_quads(tips, clv_buffers, scale_buffers, pattern_tip, rate_cats, rate_scalers, ops, count, nslots, pinned, edge4, sites,
                        quads_on, min_sites_per_class, classes, bounds, nkept, order_out, folded_out, ops_out, quads_out, counts_out,
                        products_out, bytes_out);
}

// The quad fold without a device (tests/test_host_quad_fold.py): pllhip_fused_plan_dry_quad_products, then -- fold_on --
// the step the launch takes behind it, pllhip_fused_quad_fold_walk.  qfolded_out[i] = 1: op i of the caller's list is a
// quad product its reader forms; *walked_out: the ops the kernel walks; products_out counts the folded parents with the
// walked ones, *bytes_out is of the plan that is launched.
extern "C" int pllhip_fused_plan_dry_quad_fold(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                               int pattern_tip, unsigned int rate_cats, int rate_scalers, const pllhip_op_t * ops,
                                               unsigned int count, unsigned int nslots, const unsigned char * pinned,
                                               const int * edge4, unsigned int sites, int quads_on,
                                               unsigned int min_sites_per_class, const unsigned int * classes,
                                               const double * bounds, int fold_on, unsigned int * nkept, unsigned int * order_out,
                                               unsigned char * folded_out, int * ops_out, int * quads_out,
                                               unsigned int * counts_out, unsigned char * products_out, unsigned int * bytes_out,
                                               unsigned char * qfolded_out, unsigned int * walked_out)
{
  if (!products_out || !qfolded_out || !walked_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_quad_fold: products_out, qfolded_out and walked_out");
    return -1;
  }
  return plan_dry_quads(tips, clv_buffers, scale_buffers, pattern_tip, rate_cats, rate_scalers, ops, count, nslots, pinned, edge4, sites,
                        quads_on, min_sites_per_class, classes, bounds, nkept, order_out, folded_out, ops_out, quads_out, counts_out,
                        products_out, bytes_out, fold_on, qfolded_out, walked_out);
}

extern "C" int pllhip_fused_plan_dry_deferred(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                              int pattern_tip, const pllhip_op_t * ops, unsigned int count, unsigned int nslots,
                                              const unsigned char * old_deferred, const int * old_scaler,
                                              const unsigned char * pinned, unsigned int * nkept, unsigned int * order_out,
                                              int * slots_out, int * operands_out, unsigned char * deferred_out,
                                              unsigned int * reloads_out, unsigned int * materialise_out,
                                              unsigned int * nmaterialise, unsigned int * dropped_out, unsigned int * ndropped)
{
  return plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, nslots, old_deferred, old_scaler, pinned,
                           nkept, order_out, slots_out, operands_out, deferred_out, reloads_out, materialise_out, nmaterialise,
                           dropped_out, ndropped, nullptr, 0, nullptr);
}

// The same with the edge epilogue (pllhip_ctx::edge_hint; tests/test_host_edge_fold_plan.py): the list planned by
// the driver pllhip_update_partials plans with (pllhip_fused_plan_list) as a one-segment list of a partition with
// `rate_cats` categories and per-site or no scale buffers -- unfolded at 12 waves per CU, else 8; then once more at
// that configuration with the evaluation of edge4 = {parent_clv, parent_scaler, child_clv, child_scaler} as a pseudo-op
// behind the last op.
// edge_out[8]: folded (0: the unfolded plan is what the other outputs describe), the pseudo-op's lslot (parent), rslot
// (child), lsc_slot, rsc_slot, dma_flags, workgroups per CU of the unfolded plan, of the folded one (0: not folded).
extern "C" int pllhip_fused_plan_dry_edge(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                          int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops, unsigned int count,
                                          const unsigned char * old_deferred, const int * old_scaler,
                                          const unsigned char * pinned, const int * edge4, unsigned int * nkept,
                                          unsigned int * order_out, int * slots_out, int * operands_out,
                                          unsigned char * deferred_out, unsigned int * reloads_out, int * edge_out)
{
  if (!edge4 || !edge_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_edge: no edge");
    return -1;
  }
  return plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, 0, old_deferred, old_scaler, pinned, nkept,
                           order_out, slots_out, operands_out, deferred_out, reloads_out, nullptr, nullptr, nullptr, nullptr,
                           edge4, rate_cats, edge_out);
}

// The same with pair products (pllhip_set_unstored_pairs; tests/test_host_unstored_plan.py): the list of a partition
// that may defer (pattern tips, `rate_cats` categories, no or per-site scale buffers), planned by the driver
// pllhip_update_partials plans with as one segment -- with `nslots` slots per wave, or (nslots 0) at 12 waves per CU,
// else 8 -- then pllhip_fused_unstored, the rule the live path applies.  edge4 (may be NULL): the hinted evaluation,
// as for pllhip_fused_plan_dry_edge.  unstored_out[i] = 1: op i of the caller's list is walked and its parent is not
// stored.  The other outputs are pllhip_fused_plan_dry_deferred's.
extern "C" int pllhip_fused_plan_dry_unstored(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                              int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops, unsigned int count,
                                              unsigned int nslots, const unsigned char * pinned, const int * edge4,
                                              unsigned int * nkept, unsigned int * order_out, int * slots_out,
                                              int * operands_out, unsigned char * deferred_out, unsigned int * reloads_out,
                                              unsigned char * unstored_out)
{
  if (!(rate_cats == 1 || rate_cats == 2 || rate_cats == 4) || !unstored_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_unstored: rate_cats of an instance that defers, and unstored_out");
    return -1;
  }
  int edge_out[8];
  return plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, nslots, nullptr, nullptr, pinned, nkept,
                           order_out, slots_out, operands_out, deferred_out, reloads_out, nullptr, nullptr, nullptr, nullptr,
                           edge4, rate_cats, edge_out, unstored_out);
}

// The same with folded pair products (pllhip_set_pair_fold; tests/test_host_pair_fold_plan.py): after the steps of
// pllhip_fused_plan_dry_unstored, pllhip_fused_fold picks the unstored parents with exactly one reader, an inner-inner
// op, and the list is planned once more without them.  The outputs describe that final walk: folded_out[i] = 1: op i of
// the caller's list is not walked, its reader forms the product; operands_out: 0 a slot, 1 a tip, 2 a deferred cherry,
// 3 a folded product; unstored_out: the walked ops whose parent is not stored.
extern "C" int pllhip_fused_plan_dry_folded(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                            int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops, unsigned int count,
                                            unsigned int nslots, const unsigned char * pinned, const int * edge4,
                                            unsigned int * nkept, unsigned int * order_out, int * slots_out,
                                            int * operands_out, unsigned char * deferred_out, unsigned int * reloads_out,
                                            unsigned char * unstored_out, unsigned char * folded_out)
{
  if (!(rate_cats == 1 || rate_cats == 2 || rate_cats == 4) || !unstored_out || !folded_out)
  {
    pllhip_set_error("pllhip_fused_plan_dry_folded: rate_cats of an instance that defers, unstored_out and folded_out");
    return -1;
  }
  int edge_out[8];
  return plan_dry_deferred(tips, clv_buffers, scale_buffers, pattern_tip, ops, count, nslots, nullptr, nullptr, pinned, nkept,
                           order_out, slots_out, operands_out, deferred_out, reloads_out, nullptr, nullptr, nullptr, nullptr,
                           edge4, rate_cats, edge_out, unstored_out, folded_out);
}

// The planner alone (tests/test_host.py, tools): which order and how many
// operands without a slot a list gets with `nslots` slots per wave.
extern "C" int pllhip_fused_plan_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                     int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                     unsigned int nslots, unsigned int * order_out,
                                     unsigned int * reloads_out, int * slots_out)
{
  const FusedGeom geom = {(size_t)tips + clv_buffers, scale_buffers, tips, pattern_tip != 0};
  if (dry_ops_in_range("pllhip_fused_plan_dry", geom, ops, count)) return -1;
  std::vector<PartialsArgs> args(count);
  std::vector<int> kinds(count);
  for (unsigned int i = 0; i < count; ++i) dry_resolve(geom, ops[i], args[i], kinds[i], nullptr);
  std::vector<FusedOp> plan;
  unsigned int reloads = 0;
  const int rc = pllhip_fused_plan(geom, ops, args.data(), kinds.data(), count, nslots, plan, &reloads);
  if (rc) return rc;
  for (unsigned int pos = 0; pos < count; ++pos)
  {
    if (order_out) order_out[pos] = (unsigned int)plan[pos].list_pos;
    if (slots_out) dry_slots_out(plan[pos], slots_out + (size_t)pos * 6);
  }
  if (reloads_out) *reloads_out = reloads;
  return 0;
}

// The 20-state list without a device (tests/test_host_aa_list_plan.py, test_gpu_aa_list_plan.py): the three steps
// pllhip_aa_fused_update takes before it encodes anything, on fake addresses.  incoming: the bound an earlier call left
// on each CLV (tips + clv_buffers entries; NULL: none).
// op_out[7 i ..]: op i's class (AaOpClass), its two lookup kids, whether its scaling test looks for the window, its
// segment, its position in that segment's walk and the sync-left flag (-1 / -1 / 0: ahead of the list).
// list_out[14]: list_ti_mfma, cert_kind, cert_too_wide, reloads, segments, ops walked, pllhip_aa_list_kinds' eight.
// bounds_out (tips + clv_buffers): `incoming` with what the list leaves marked.  Any output may be NULL.
// Returns 0, 1 if the kernel does not take the list (op_out holds the classes if it got that far), -1 on bad indices.
extern "C" int pllhip_aa_list_plan_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                       int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                       unsigned int lookups_max, int tt_inside, int ti_mfma, unsigned int max_segments,
                                       const double * incoming, int * op_out, int * list_out, double * window_out,
                                       double * bounds_out)
{
  const FusedGeom geom = {(size_t)tips + clv_buffers, scale_buffers, tips, pattern_tip != 0};
  if (dry_ops_in_range("pllhip_aa_list_plan_dry", geom, ops, count)) return -1;
  std::vector<PartialsArgs> args(count);
  std::vector<int> kinds(count), scales(count);
  for (unsigned int i = 0; i < count; ++i)
  {
    dry_resolve(geom, ops[i], args[i], kinds[i], nullptr);
    scales[i] = ops[i].parent_scaler >= 0;
  }
  for (unsigned int t = 0; list_out && t < 14; ++t) list_out[t] = 0;
  for (unsigned int t = 0; op_out && t < 7 * count; ++t) op_out[t] = t % 7 == 0 || t % 7 == 3 || t % 7 == 6 ? 0 : -1;
  AaListClasses lc;
  if (pllhip_aa_list_classify(geom, ops, kinds.data(), scales.data(), count, lookups_max, tt_inside != 0 && pattern_tip, lc)) return 1;
  AaListCert cert;
  pllhip_aa_list_cert(geom, ops, lc.cls.data(), count, incoming, ti_mfma != 0, cert);
  for (unsigned int i = 0; op_out && i < count; ++i)
  {
    const int v[4] = {lc.cls[i], lc.lk_kids[i].first, lc.lk_kids[i].second, cert.op_inexact[i]};
    memcpy(op_out + 7 * (size_t)i, v, sizeof(v));
  }
  if (window_out) *window_out = cert.window;
  for (size_t i = 0; bounds_out && i < geom.nclv; ++i) bounds_out[i] = incoming ? incoming[i] : 0.0;
  for (const auto & m : cert.out_marks)
    if (bounds_out) bounds_out[m.first] = m.second;
  AaListWalk walk;
  const int rc = pllhip_aa_list_walk(geom, ops, args.data(), lc.cls.data(), scales.data(), count, max_segments,
                                     PLLHIP_AA_FUSED_SLOTS, walk);
  if (list_out)
  {
    const int v[6] = {cert.list_ti_mfma, cert.cert_kind, cert.too_wide, (int)walk.reloads, rc ? 0 : (int)walk.nsegs,
                      rc ? 0 : (int)walk.plan.size()};
    memcpy(list_out, v, sizeof(v));
    unsigned int k8[8];
    pllhip_aa_list_kinds_of(lc.cls.data(), count, cert.list_ti_mfma, walk.reloads, k8);
    for (int t = 0; t < 8; ++t) list_out[6 + t] = (int)k8[t];
  }
  if (rc) return rc;
  for (unsigned int sg = 0; op_out && sg < walk.nsegs; ++sg)
    for (unsigned int pos = 0; pos < walk.seg_n[sg]; ++pos)
    {
      const unsigned int at = walk.seg_first[sg] + pos;
      int * o = op_out + 7 * (size_t)walk.orig[walk.plan[at].list_pos];
      o[4] = (int)sg;
      o[5] = (int)pos;
      o[6] = walk.sync_left[at];
    }
  return 0;
}

// Where each op's tip characters sit in a wave's character registers.  A wave holds the characters of 64 / lpr tip
// rows of its tile at a time (lpr lanes of 16 bytes per row); the rows are dealt in the order the list uses them,
// both rows of an op into the same batch.  tips[pos]: bit 0 / 1 = the op has a left / right tip.  Out, per op:
// chars (PLLHIP_FUSED_CH_LPOS / RPOS = first lane of the row, CH_LTIP / CH_RTIP) and the batch its rows are in
// (an op without tips: the batch current at that point).  Returns the number of batches.  Pure host logic.
unsigned int pllhip_fused_char_batches8(const unsigned int * tips, unsigned int count, unsigned int lpr,
                                        unsigned int * const chars_out[4], unsigned int * batch_out)
{
  const unsigned int rpb = 64 / lpr; // rows per batch
  unsigned int batch = 0, q = 0;
  for (unsigned int pos = 0; pos < count; ++pos)
  {
    unsigned int n = 0;
    for (int b = 0; b < 8; ++b) n += (tips[pos] >> b) & 1u;
    if (q + n > rpb)
    {
      ++batch;
      q = 0;
    }
    batch_out[pos] = batch;
    // (all the rows of an op lie in one batch, in the order of its gathers)
    for (int k = 0; k < 4 && chars_out[k]; ++k)
    {
      chars_out[k][pos] = 0;
      if (tips[pos] & (1u << (2 * k))) chars_out[k][pos] |= PLLHIP_FUSED_CH_LTIP | (q++ * lpr);
      if (tips[pos] & (2u << (2 * k))) chars_out[k][pos] |= PLLHIP_FUSED_CH_RTIP | (q++ * lpr) << 8;
    }
  }
  return batch + 1;
}

unsigned int pllhip_fused_char_batches(const unsigned int * tips, unsigned int count, unsigned int lpr,
                                       unsigned int * chars_out, unsigned int * batch_out)
{
  // (two rows per op: bits 0 / 1 of tips[pos] only)
  std::vector<unsigned int> two(tips, tips + count);
  for (unsigned int & t : two) t &= 3u;
  unsigned int * const out[4] = {chars_out, nullptr, nullptr, nullptr};
  return pllhip_fused_char_batches8(two.data(), count, lpr, out, batch_out);
}

extern "C" unsigned int pllhip_fused_char_batches_dry(const unsigned int * tips, unsigned int count, unsigned int rate_cats,
                                                      unsigned int * chars_out, unsigned int * batch_out)
{
  const unsigned int ts = PLLHIP_FUSED_J * (64 / (2 * rate_cats));
  return pllhip_fused_char_batches(tips, count, ts >= 16 ? ts / 16 : 1, chars_out, batch_out);
}

// Independent sub-lists (FusedSeg in partials_fused.hpp).  Two ops belong together when one of them writes a
// buffer -- CLV or scale buffer -- the other reads or writes; buffers nobody in the list writes (tips, operands of
// earlier calls) tie nothing.  Union-find over the ops, then the components dealt longest first.
unsigned int pllhip_fused_segments(const FusedGeom & geom, const pllhip_op_t * ops, unsigned int count,
                                   unsigned int max_segments, std::vector<unsigned int> & seg_of)
{
  seg_of.assign(count, 0u);
  if (max_segments > PLLHIP_FUSED_MAX_SEGS) max_segments = PLLHIP_FUSED_MAX_SEGS;
  if (count < 4 || max_segments < 2) return 1;
  // (every new list passes here: the work arrays are the thread's, not the heap's)
  static thread_local std::vector<unsigned int> parent, size, roots, load, seg_of_root;
  static thread_local std::vector<int> clv_first, sc_first;
  parent.resize(count);
  for (unsigned int i = 0; i < count; ++i) parent[i] = i;
  auto find = [&](unsigned int x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  auto join = [&](unsigned int a, unsigned int b) {
    a = find(a);
    b = find(b);
    if (a != b) parent[a > b ? a : b] = a < b ? a : b;
  };
  // first op that touches each WRITTEN buffer (-1: not written in this list, -2: written, nobody met yet)
  clv_first.assign(geom.nclv, -1);
  sc_first.assign(geom.nsc, -1);
  for (unsigned int i = 0; i < count; ++i)
  {
    if (ops[i].parent_clv >= geom.nclv || ops[i].child1_clv >= geom.nclv || ops[i].child2_clv >= geom.nclv ||
        ops[i].parent_scaler >= (int)geom.nsc || ops[i].child1_scaler >= (int)geom.nsc || ops[i].child2_scaler >= (int)geom.nsc)
      return 1; // (the path taken reports it)
    clv_first[ops[i].parent_clv] = -2;
    if (ops[i].parent_scaler >= 0) sc_first[ops[i].parent_scaler] = -2;
  }
  for (unsigned int i = 0; i < count; ++i)
  {
    auto touch = [&](std::vector<int> & first, int idx) {
      if (idx < 0 || first[idx] == -1) return;
      if (first[idx] == -2) first[idx] = (int)i;
      else join((unsigned int)first[idx], i);
    };
    touch(clv_first, (int)ops[i].parent_clv);
    touch(clv_first, (int)ops[i].child1_clv);
    touch(clv_first, (int)ops[i].child2_clv);
    touch(sc_first, ops[i].parent_scaler);
    touch(sc_first, ops[i].child1_scaler);
    touch(sc_first, ops[i].child2_scaler);
  }
  // components by size, longest first (ties: the one that begins first)
  size.assign(count, 0u);
  for (unsigned int i = 0; i < count; ++i) ++size[find(i)];
  roots.clear();
  for (unsigned int i = 0; i < count; ++i)
    if (size[i]) roots.push_back(i);
  if (roots.size() < 2) return 1;
  std::stable_sort(roots.begin(), roots.end(), [&](unsigned int a, unsigned int b) { return size[a] > size[b]; });
  // as many segments as have two ops each at least, and no more than shorten the longest
  unsigned int nsegs = (unsigned int)std::min<size_t>(max_segments, roots.size());
  seg_of_root.assign(count, 0u);
  for (;; --nsegs)
  {
    load.assign(nsegs, 0u);
    for (unsigned int r : roots)
    {
      const unsigned int k = (unsigned int)(std::min_element(load.begin(), load.end()) - load.begin());
      seg_of_root[r] = k;
      load[k] += size[r];
    }
    if (nsegs == 1 || *std::min_element(load.begin(), load.end()) >= 2) break;
  }
  if (nsegs == 1) return 1;
  // segment 0 the longest, as the header says and the kernels' segment-major order wants (every tile of the longest
  // segment first): the greedy dealing above does not give that by itself once components outnumber segments --
  // components of 5, 4 and 4 ops over two segments are loads of 5 and 8 -- so the segments are numbered by
  // descending load afterwards (tests/test_host.py)
  std::vector<unsigned int> rank_of(nsegs);
  {
    std::vector<unsigned int> by_load(nsegs);
    for (unsigned int k = 0; k < nsegs; ++k) by_load[k] = k;
    std::stable_sort(by_load.begin(), by_load.end(), [&](unsigned int a, unsigned int b) { return load[a] > load[b]; });
    for (unsigned int r = 0; r < nsegs; ++r) rank_of[by_load[r]] = r;
  }
  for (unsigned int i = 0; i < count; ++i) seg_of[i] = rank_of[seg_of_root[find(i)]];
  return nsegs;
}

extern "C" unsigned int pllhip_fused_segments_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                  int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                                  unsigned int max_segments, unsigned int * seg_out)
{
  const FusedGeom geom = {(size_t)tips + clv_buffers, scale_buffers, tips, pattern_tip != 0};
  std::vector<unsigned int> seg_of;
  const unsigned int n = pllhip_fused_segments(geom, ops, count, max_segments, seg_of);
  for (unsigned int i = 0; i < count && seg_out; ++i) seg_out[i] = seg_of[i];
  return n;
}
