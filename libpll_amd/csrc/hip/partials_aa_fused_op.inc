// partials_aa_fused_op.inc -- ONE op of k_aa_fused (partials_aa_fused.hip), included twice with the two
// record variables swapped (AF_RC: this op's record, AF_RN: where the next one is loaded to): a
// loaded value is never copied -- a copy would have to wait for its load.  Not a lambda: the slot
// variables must never have their address taken.
//
// The pipeline.  Vector-memory operations return IN ORDER, stores included, and a store of this
// kernel is acknowledged only microseconds after it was issued (the chip is writing at its limit).
// So nothing an op waits for may be requested behind a store: everything op i + 1 needs from
// memory is requested at the end of op i BEFORE the six stores of op i --
//   its right block and the left block of op i + 2 (LDS: one right block, two left blocks in turn),
//   a lookup's table entries (LDS-DMA gathers into the wave's two stages) or a tip's table row,
//   the characters of op i + 2 --
// and waited for with vmcnt(7): "all but my six stores (and the character load issued since)".
//   first half    left products (left block: landed before barrier A of op i - 1; behind a lookup, which has no
//                 barriers, the op begins with one of its own)
//   barrier A     the right block has landed everywhere
//   second half   right products, product, scaling (a lookup: multiply the two stages)
//   barrier B     everybody is done with the right block  (nothing to wait for)
//   second half   ... then the parent's slot and the transposition through stage 0 (the wave's own)
//   end           requests for the ops ahead, six stores
{
  const unsigned int fl = __builtin_amdgcn_readfirstlane(AF_RC[18]);
  const unsigned int kind = fl & AF_KIND_MASK;
  const unsigned int slots = __builtin_amdgcn_readfirstlane(AF_RC[19]);
  const bool scaling = MODE != SCALE_NONE && (fl & AF_SCALING);
  const bool last = (fl & AF_LAST) != 0u;
  // the next op's record (the records are linked and the list is cyclic: the next tile begins with op 0)
  AF_RN = af_load<0, 28>(plan, fl >> AF_NEXT_SHIFT);
  const char * xlane = (xpar ? x1lane : x0lane);
  // the characters of op i + 2 (whose rows THIS op's record names), behind the six
  // stores of op i - 1 and ahead of everything this op requests: nobody waits for them before the end
  // of op i + 1, and a wait for "all but my six stores" becomes "all but my six stores and one character load"
  request_chars(AF_RC, AF_CH_REQ);

  // ---- first half
  // (an inner-inner op fetches what the next op reloads while it multiplies; a tip-inner op and a lookup keep
  // both stages busy until their products are done and fetch it then, one after the other)
  unsigned int ra_cj[AF_J] = {0u, 0u}, rb_cj[AF_J] = {0u, 0u};
  if ((fl & AF_RELOAD_A) && kind == 0u)
  {
    reload_issue(AF_RC.quad(20));
    reload_counts(AF_RC.quad(22), ra_cj);
  }
  double x[AF_J][5];       // the left factor, then the product
  unsigned int lc[AF_J], rcn[AF_J];
#pragma unroll
  for (int j = 0; j < AF_J; ++j) lc[j] = rcn[j] = 0u;
  // (x is given a value on every path: a variable that is not keeps its value of the op before alive
  // across the whole loop as far as the register allocator is concerned -- seen: 20 registers, spilled)
  if (kind == 0u)
  {
    // (behind a lookup, which has no barrier: everybody's part of the left block has landed once everybody is
    // here -- each wave waited for its own part at the lookup's vmcnt wait)
    if (fl & AF_SYNC_LEFT) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    AfSlot l;
    AF_SLOT_READ(slots & 15u, l)
#pragma unroll
    for (int j = 0; j < AF_J; ++j) lc[j] = l.c[j];
    const unsigned int lm = lane_again();
    af_matvec<false>(xlane, xlane - lm * 8u + cls32_of(lm), lm, l.v, x);
  }
  else
  {
    // (a tip-inner op: the tip's factor -- a row of its table per site -- was gathered into stage 1 during the op
    // before, ahead of that op's stores, and stays there until af_matvec_plain multiplies by it)
#pragma unroll
    for (int j = 0; j < AF_J; ++j)
#pragma unroll
      for (int t = 0; t < 5; ++t) x[j][t] = 0.0;
  }
  if ((fl & AF_RELOAD_A) && kind == 0u) AF_RELOAD_TAKE((slots >> 12) & 15u, ra_cj)

  // ---- barrier A: all but my six stores have arrived (the right block with them, and a tip's factor)
  if ((fl & AF_RELOAD_A) && kind == 0u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  // (a lookup multiplies by no block: it needs neither barrier and the waves may drift apart over
  // it -- which also keeps their requests from colliding.  What it requests for the ops ahead goes to
  // buffers whose last readers were through before a barrier every wave has passed.)
  if (kind <= 1u) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // the left block of op i + 2 into this op's left buffer, which everybody is done with: requested here,
  // not with the rest at the end -- the waves of a workgroup run in lock-step and their requests collide
  {
    const unsigned int nnkind = (__builtin_amdgcn_readfirstlane(AF_RN[18]) >> 8) & AF_KIND_MASK;
    if (nnkind == 0u) stage_matrix(xpar ? x1buf_b : x0buf_b, AF_RN[16]);
  }
  // Round 4: what the next op gathers, EARLY -- when that is one row per site of a single table (a tip-tip op's pair
  // table: into stage 1) and this op leaves stage 1 alone from here on (an inner-inner op that reloads no right
  // operand: it transposes through stage 0).  The gather then lands while this op multiplies, instead of being issued
  // with the block requests and the stores at the op's end, where the four waves of the workgroup queue on the
  // texture path, and being waited for at the top of the next op.
  const bool early_gather = kind == 0u && !(fl & AF_RELOAD_B) && !last &&
                            (__builtin_amdgcn_readfirstlane(AF_RN[18]) & (AF_KIND_MASK | AF_ONE_TABLE)) == (2u | AF_ONE_TABLE);
  if (early_gather)
  {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // (stage 1's last readers -- a reload's -- are done)
    next_gathers(2u, true, AF_RN.quad(4), AF_RN.quad(6), AF_CH_USE);
  }
  if ((fl & AF_RELOAD_B) && kind == 0u)
  {
    reload_issue(AF_RC.quad(24));
    reload_counts(AF_RC.quad(26), rb_cj);
  }

  // ---- second half
  double2 g[5];            // the finished tile, 16 bytes per lane: granule it * 64 + lane
  unsigned int pc[AF_J];   // the parent's counts, lane's own site of each sub-tile
  if (kind <= 1u)
  {
    AfSlot p;              // the parent in the operand layout (what its slot takes)
    {
      AfSlot r;
      AF_SLOT_READ((slots >> 4) & 15u, r)
#pragma unroll
      for (int j = 0; j < AF_J; ++j) rcn[j] = r.c[j];
      if (kind == 1u && !(fl & AF_TI_MFMA))
      {
        // (yrows: the right block in row order, the lane's class x 16 bytes)
        const unsigned int lm = lane_again();
        af_matvec_plain(st0 + boff, st0 + boff5, st0 + coloff_of(lm), lds + 2 * AF_MAT_B + cls32_of(lm) / 2u, st1 + boff, st1 + boff5, r.v, x);
      }
      else
      {
        // (an inner-inner op -- or, opt-in, a tip-inner op on the matrix cores: x = the tip's factor, gathered into
        // stage 1 during the op before, times the fused chains; its block was staged in operand order)
        if (kind == 1u) af_read_tile(st1 + boff, st1 + boff5, x);
        const unsigned int lm = lane_again();
        af_matvec<true>(ylane, ylane - lm * 8u + cls32_of(lm), lm, r.v, x);
      }
    }
    // Round 6, the scaling certificate (AF_CERT: an op whose value may carry the matrix cores' rounding of a tip-inner
    // mat-vec from further down the tree -- 1e-15 relative per op -- and whose scaling decision must nevertheless be the
    // reference's): a decision can differ only when the largest entry lies within that error of the threshold.  The test
    // in the op loop is two integer instructions on the high word of the lane's largest entry (a window of 2^-20); only
    // when a lane passes it -- once in millions of ops -- does the wave fetch the call's window from the segment's header
    // (words 2-3: 2^-256 x the relative half-width as a double) and, inside it, raise the call's flag (words 0-1: a word
    // in host memory).  The host re-runs the list in the reference's order then (partials.hip: pllhip_cert_resolve).
    if (scaling && (fl & AF_CERT))
    {
      double mx[AF_J];
      bool wide = false;
#pragma unroll
      for (int j = 0; j < AF_J; ++j)
      {
        mx[j] = fmax(fmax(fmax(x[j][0], x[j][1]), fmax(x[j][2], x[j][3])), x[j][4]);
        wide = wide || ((unsigned int)__double2hiint(mx[j]) - 0x2FEFFFFFu) < 2u;
      }
      if (__ballot(wide))
      {
        const AfW<0, 4> hh = af_load<0, 4>(plan, cur_rec0);
        const double w = __hiloint2double((int)hh[3], (int)hh[2]);
        bool inside = false;
#pragma unroll
        for (int j = 0; j < AF_J; ++j) inside = inside || fabs(mx[j] - PLLHIP_SCALE_THRESHOLD) < w;
        if (__ballot(inside) && lane == 0u) *(unsigned int PLL_GLOBAL *)af_base(hh.quad(0)) = 1u;
      }
    }
#pragma unroll
    for (int j = 0; j < AF_J; ++j)
    {
      bool small = true;
#pragma unroll
      for (int t = 0; t < 5; ++t)
      {
        p.v[j][t] = x[j][t];
        small = small && (p.v[j][t] < PLLHIP_SCALE_THRESHOLD);
      }
      // scaling rule of core_partials_avx2.c:752-800: every entry of the site below the threshold -- or, with a scale
      // buffer per rate category (core_partials_avx.c:494-503), every entry of the site's block of that category: in
      // this layout the four lanes q of one (rate, site)
      unsigned int scaled = 0u;
      if (scaling)
      {
        const unsigned long long bal = __ballot(small);
        const unsigned long long m = MODE == SCALE_RATE ? 0x0001000100010001ull << (lane & 15u) : 0x1111111111111111ull << n;
        scaled = (bal & m) == m ? 1u : 0u;
        if (__ballot(scaled != 0u))
        {
          const double f = scaled ? PLLHIP_SCALE_FACTOR : 1.0;
#pragma unroll
          for (int t = 0; t < 5; ++t) p.v[j][t] *= f;
        }
      }
      pc[j] = scaling ? ((fl & AF_LCNT) ? lc[j] : 0u) + ((fl & AF_RCNT) ? rcn[j] : 0u) + scaled : 0u;
      p.c[j] = pc[j];
    }
    // the tile into the layout of the stores, through stage 0 (the wave's own: no barrier involved)
#pragma unroll
    for (int j = 0; j < AF_J; ++j)
    {
      *reinterpret_cast<double2 *>(st0 + boff + j * 2560) = make_double2(p.v[j][0], p.v[j][1]);
      *reinterpret_cast<double2 *>(st0 + boff + j * 2560 + 16) = make_double2(p.v[j][2], p.v[j][3]);
      *reinterpret_cast<double *>(st0 + boff5 + j * 2560) = p.v[j][4];
    }
    asm volatile("" ::: "memory");
    // the parent's slot (slot 15 is nobody's: no branch)
    AF_SLOT_WRITE((fl & AF_HAS_PSLOT) ? (slots >> 8) & 15u : 15u, p)
#pragma unroll
    for (int it = 0; it < 5; ++it) g[it] = *reinterpret_cast<const double2 *>(st0 + it * 1024 + lane16);
    asm volatile("" ::: "memory");
  }
  else
  {
    // lookup: parent = TL[pair 1] (.) TR[pair 2] (k_aa_cherry_rounds, partials_aa_mfma.hip); the
    // entries were gathered into the two stages during the op before, in the layout of the stores
    unsigned long long bal[5];
    if (fl & AF_ONE_TABLE)
    {
      // (a tip-tip op's pair table: the product was made when the table was, k_af_prepare; it never scales)
#pragma unroll
      for (int it = 0; it < 5; ++it)
      {
        g[it] = *reinterpret_cast<const double2 *>(st1 + it * 1024 + lane16);
        bal[it] = 0ull;
      }
    }
    else
    {
#pragma unroll
      for (int it = 0; it < 5; ++it)
      {
        const double2 a = *reinterpret_cast<const double2 *>(st0 + it * 1024 + lane16);
        const double2 b = *reinterpret_cast<const double2 *>(st1 + it * 1024 + lane16);
        g[it] = make_double2(a.x * b.x, a.y * b.y);
        bal[it] = __ballot((g[it].x < PLLHIP_SCALE_THRESHOLD) & (g[it].y < PLLHIP_SCALE_THRESHOLD));
      }
    }
    // bit s: every entry of site s of the tile below the threshold.  The 320 flags of the tile
    // are five wave masks; site s owns bits [40 s, 40 s + 40).  (Nearly always no flag is set.)
    // Per-rate scale buffers: bit 4 s + r, the ten flags [40 s + 10 r, + 10) of category r's block.
    unsigned int scaled = 0u;
    if (scaling && (bal[0] | bal[1] | bal[2] | bal[3] | bal[4]) != 0ull)
    {
      if (MODE == SCALE_RATE)
      {
#pragma unroll
        for (int b = 0; b < 4 * AF_WS; ++b)
        {
          const int w = (10 * b) / 64, off = (10 * b) % 64;
          unsigned long long field = bal[w] >> off;
          if (off > 54) field |= bal[w + 1 < 5 ? w + 1 : 4] << (64 - off);
          scaled |= ((field & 0x3ffull) == 0x3ffull) ? 1u << b : 0u;
        }
      }
      else
      {
#pragma unroll
        for (int s = 0; s < AF_WS; ++s)
        {
          constexpr unsigned long long F40 = (1ull << 40) - 1ull;
          const int w = (40 * s) / 64, off = (40 * s) % 64;
          unsigned long long field = bal[w] >> off;
          if (off > 24) field |= bal[w + 1 < 5 ? w + 1 : 4] << (64 - off);
          scaled |= ((field & F40) == F40) ? 1u << s : 0u;
        }
      }
      scaled = __builtin_amdgcn_readfirstlane(scaled);
      if (scaled)
      {
        unsigned int lane_l = lane;
        asm volatile("" : "+v"(lane_l));
#pragma unroll
        for (unsigned int it = 0; it < 5; ++it)
        {
          const unsigned int sl = (it * 64u + lane_l) / (MODE == SCALE_RATE ? 10u : 40u);
          const double f = ((scaled >> sl) & 1u) ? PLLHIP_SCALE_FACTOR : 1.0;
          g[it].x *= f;
          g[it].y *= f;
        }
      }
    }
    // (both children are tip-tip results: nothing to inherit)
#pragma unroll
    for (int j = 0; j < AF_J; ++j) pc[j] = MODE == SCALE_RATE ? (scaled >> ((4 * j + n) * 4 + rate)) & 1u : (scaled >> (4 * j + n)) & 1u;
    // When the parent has a slot it is needed in the operand layout too.  A single table's rows (a tip-tip op: no
    // product, no scaling) ARE in stage 1 in the layout of a CLV: the operand layout is read straight from there.
    // Two tables: the finished tile goes through stage 0, five conflict-free writes and six reads.  (Reading both
    // factors in the operand layout instead and multiplying once more -- no round trip through LDS -- was measured in
    // round 4 and is slower, C3 1.790 -> 1.808 ms: the operand-layout reads are the ones with bank conflicts.)
    if (fl & AF_HAS_PSLOT)
    {
      // (the tile's way into the slot differs, the slot's write does not -- but a value that two paths produce and one
      // statement consumes is twenty registers kept alive across both: the kernel spilled.  Stage and offset are
      // chosen instead, wave-uniformly, and ONE sequence reads the tile.)
      const bool direct = (fl & AF_ONE_TABLE) != 0u;
      if (!direct)
      {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int it = 0; it < 5; ++it) *reinterpret_cast<double2 *>(st0 + it * 1024 + lane16) = g[it];
        asm volatile("" ::: "memory");
      }
      const char * from = direct ? st1 : st0;
      AfSlot p;
      af_read_tile(from + boff, from + boff5, p.v);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int j = 0; j < AF_J; ++j) p.c[j] = pc[j];
      AF_SLOT_WRITE((slots >> 8) & 15u, p)
    }
  }
  if (kind != 0u)
  {
    // (the stages were busy until here: what the next op reloads is fetched now, one after the other)
    if (fl & AF_RELOAD_A)
    {
      reload_issue(AF_RC.quad(20));
      reload_counts(AF_RC.quad(22), ra_cj);
      AF_RELOAD_TAKE((slots >> 12) & 15u, ra_cj)
    }
    if (fl & AF_RELOAD_B)
    {
      reload_issue(AF_RC.quad(24));
      reload_counts(AF_RC.quad(26), rb_cj);
    }
  }
  if (fl & AF_RELOAD_B) AF_RELOAD_TAKE((slots >> 16) & 15u, rb_cj)

  // ---- barrier B: everybody is done with the right block (and with this op's left block)
  if (kind <= 1u) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- requests for the ops ahead, all of them BEFORE this op's stores
  {
    const unsigned int nfl = __builtin_amdgcn_readfirstlane(AF_RN[18]);
    const unsigned int nkind = nfl & AF_KIND_MASK;
    // (the stages are free: their readers are done)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (nkind <= 1u) stage_matrix(ybuf_b, AF_RN[17]);
    // what op i + 1 gathers -- unless it belongs to the next tile (other sites: the prologue does it)
    if (!last && !early_gather) next_gathers(nkind, (nfl & AF_ONE_TABLE) != 0u, AF_RN.quad(4), AF_RN.quad(6), AF_CH_USE);
  }
  asm volatile("" ::: "memory");
  // the six stores (always six: barrier A of the next op counts on it): the counts -- to the wave's sink
  // when the op has no scale buffer --, then the tile, 5 KB contiguous
  {
    // (lane offsets through an empty asm: extended to 64 bits outside the loop they are not folded into
    // the "scalar base + 32-bit lane offset" form of the instruction any more, and cost register pairs)
    // (and formed here from the lane number, not carried through the loop: kept across the op, `lane * 4` was the
    // register the compiler parked in a0 -- a slot -- during the vector-unit mat-vec, tools/check_agprs.py)
    unsigned int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    const unsigned int lane4 = lane_s * 4u, lane16s = lane_s * 16u;
    unsigned int mine = (lane & 4u) ? pc[1] : pc[0];
    if (MODE == SCALE_RATE)
    {
      // entry (site, rate) of the scale buffer = lane 4 site + rate of the store; the count sits in lane (rate, n) of
      // pc[site >> 2]: a transposition of the first sixteen lanes through the LDS crossbar
      const unsigned int from = ((lane_s & 3u) * 4u + ((lane_s >> 2) & 3u)) * 4u;
      const unsigned int v0 = (unsigned int)__builtin_amdgcn_ds_bpermute((int)from, (int)pc[0]);
      const unsigned int v1 = (unsigned int)__builtin_amdgcn_ds_bpermute((int)from, (int)pc[1]);
      mine = (lane & 16u) ? v1 : v0;
    }
    // (a tip-tip op of the list never scales and has pc = 0: it clears its scale buffer)
    const af_gptr cdst = af_base((scaling || (MODE != SCALE_NONE && (fl & AF_ZERO_COUNTS))) ? AF_RC.quad(2) + cnt_off : sink_a);
    asm volatile("" ::: "memory");
    if (lane < (MODE == SCALE_RATE ? 4u : 1u) * (unsigned int)AF_WS) *(unsigned int PLL_GLOBAL *)(cdst + lane4) = mine;
    asm volatile("" ::: "memory");
    const af_gptr out = af_base(AF_RC.quad(0) + clv_off);
#pragma unroll
    for (unsigned int it = 0; it < 5; ++it)
    {
      const pll_v2d v = {g[it].x, g[it].y};
      pll_v2d PLL_GLOBAL * dst = (pll_v2d PLL_GLOBAL *)(out + (lane16s + it * 1024u));
      if (NT) __builtin_nontemporal_store(v, dst);
      else *dst = v;
      asm volatile("" ::: "memory");
    }
  }
  xpar ^= 1u;
  af_last = last;
}
