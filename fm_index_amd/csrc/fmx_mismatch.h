// fmx_mismatch.h -- batched backward search with up to FMX_MAX_MISMATCHES substitutions on the 32-bit engine
// (fmx_mismatch_count_batch* / fmx_mismatch_search_batch*; included by fmx_query.hip).
//
// An ADDITION with no counterpart in the crate.  For pattern P of m symbols and budget K (include/fmx.h):
//     enum(i, s, e, d):                      # i symbols still to prepend, d substitutions spent
//         if i == 0: emit (s, e, edits); return
//         p = P[i-1]
//         if d < K:
//             for c = 1 .. max_character ascending, c != p:
//                 s' = lf_map2(c, s); e' = lf_map2(c, e)
//                 if e' > s': enum(i-1, s', e', d+1)   # edit (pos = i-1, sym = c) appended
//         if p <= max_character:
//             s' = lf_map2(p, s); e' = lf_map2(p, e)
//             if e' > s': enum(i-1, s', e', d)
// The recursion is walked depth-first by ONE 8-lane group per pattern, as a flat loop: every trip of the loop makes at
// most one pair of record requests, whatever level of the recursion the group's pattern is in, so the eight groups of
// a wave stay in step.  At most K frames (levels with d < K) are live; they are named registers, unrolled on K.
// The same kernel body serves both passes: WRITE = false counts the intervals and their rows, WRITE = true writes
// interval j of pattern k to slot out_off[k] + j -- only while that slot is below min(out_off[k + 1], total) -- and
// reports FMX_ERR_ARG when the pattern emits more or fewer intervals than its slots.
//
// The accelerators (pair index, k-mer table) are not used: they cannot place a substitution inside a pair or a k-mer.
#pragma once

// what a pattern reads before its first step; returns false when the pattern must not be read (bad offsets / range:
// FMX_ERR_ARG is set) or holds no row.  Shared by every kernel below.
__device__ __forceinline__ bool fmx_mm_begin(const uint64_t *__restrict__ off, const uint64_t *__restrict__ s0e0,
                                             uint64_t k, uint64_t pmin, uint64_t ptot, uint32_t n, uint32_t *status,
                                             uint32_t g, uint64_t &pbeg, uint32_t &m, uint32_t &s, uint32_t &e) {
  pbeg = off[k];
  const uint64_t pend = off[k + 1];
  m = (uint32_t)(pend - pbeg);
  // offsets that go backwards or leave the pattern buffer: refuse, do not read
  bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
  s = 0; e = n;
  if (s0e0) {
    const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
    s = (uint32_t)s64;
    e = (uint32_t)e64;
    bad |= s64 > n || e64 > n;                           // not a range of this index
  }
  if (bad && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
  return !bad && e > s;
}

// the slots of pattern k in pass 2: [base, base + room) with room cut at min(out_off[k + 1], total)
struct FmxMmSlots { uint64_t base, top, room; };
__device__ __forceinline__ FmxMmSlots fmx_mm_slots(const uint64_t *__restrict__ out_off, uint64_t k, uint64_t total) {
  FmxMmSlots r;
  r.base = out_off[k];
  r.top = out_off[k + 1];
  const uint64_t lim = r.top < total ? r.top : total;
  r.room = lim > r.base ? lim - r.base : 0;
  return r;
}
// interval number `j` of a pattern (pass 2); a slot outside the pattern's own is never written
__device__ __forceinline__ void fmx_mm_emit(const FmxMmSlots &sl, uint64_t j, uint32_t s, uint32_t e, uint32_t d,
                                            uint64_t ed0, uint64_t ed1, uint64_t *__restrict__ out_s,
                                            uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  if (j < sl.room) {
    const uint64_t slot = sl.base + j;
    if (out_s) out_s[slot] = s;
    if (out_e) out_e[slot] = e;
    if (out_edit) {
      out_edit[2 * slot] = d > 0 ? ed0 : ~0ull;
      out_edit[2 * slot + 1] = d > 1 ? ed1 : ~0ull;
    }
  }
}
// end of a pattern: pass 1 stores its totals, pass 2 compares the intervals it emitted with its slots
template <bool WRITE>
__device__ __forceinline__ void fmx_mm_finish(const FmxMmSlots &sl, uint64_t k, uint64_t total, uint64_t nint,
                                              uint64_t rows, uint32_t *status, uint64_t *__restrict__ out_nint,
                                              uint64_t *__restrict__ out_cnt) {
  if (WRITE) {
    if (sl.top < sl.base || sl.top > total || sl.top - sl.base != nint) atomicOr(status, 1u << FMX_ERR_ARG);
  } else {
    if (out_nint) out_nint[k] = nint;
    if (out_cnt) out_cnt[k] = rows;
  }
}

// group per pattern, every kind and level count: one fmx_lf_map2_pair per candidate symbol and trip of the loop, so
// the cost of a frame grows with the alphabet (symbols that do not occur in the text are skipped eight at a time from
// the C array: their interval is empty either way).  The correct-everywhere path, not the fast one.
template <int KIND, int NL, int SM, bool WRITE>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_mm_kernel(
    FmxDev ix, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint32_t K, const uint64_t *__restrict__ out_off, uint64_t total,
    uint64_t *__restrict__ out_nint, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol
  const uint32_t maxc = ix.max_character;
  // entries of the structure the C array counts: rows (FM, multi-pieces) or runs (RLFM)
  const uint32_t ctot = KIND == FMX_KIND_RLFM ? ix.bw.len : ix.n;

  uint64_t k = gid, pbeg = 0, nint = 0, rows = 0;
  bool active = k < npat, fresh = true;
  // frame of level t (t substitutions spent): i symbols still to prepend, its interval, the symbol P[i - 1] and the
  // next candidate symbol (maxc + 1: the pattern's own symbol is next; level K has no candidates)
  uint32_t fi0 = 0, fs0 = 0, fe0 = 0, fp0 = 0, fc0 = 0;
  uint32_t fi1 = 0, fs1 = 0, fe1 = 0, fp1 = 0, fc1 = 0;
  uint32_t fi2 = 0, fs2 = 0, fe2 = 0, fp2 = 0;
  uint64_t ed0 = 0, ed1 = 0;
  int d = 0;                                     // current level; -1: the pattern is finished
  FmxMmSlots sl{0, 0, 0};
  while (active) {
    if (fresh) {
      uint32_t m, s, e;
      nint = 0; rows = 0;
      if (WRITE) sl = fmx_mm_slots(out_off, k, total);
      const bool go = fmx_mm_begin(off, s0e0, k, pmin, ptot, ix.n, ix.status, g, pbeg, m, s, e);
      d = go ? 0 : -1;
      fi0 = m; fs0 = s; fe0 = e; fc0 = 1;
      fp0 = (go && m) ? fmx_load_sym(pat, ix.sym_bytes, pbeg + m - 1) : 0u;
      fresh = false;
    }
    if (d >= 0) {
      const uint32_t i = d == 0 ? fi0 : (d == 1 ? fi1 : fi2), s = d == 0 ? fs0 : (d == 1 ? fs1 : fs2),
                     e = d == 0 ? fe0 : (d == 1 ? fe1 : fe2), p = d == 0 ? fp0 : (d == 1 ? fp1 : fp2);
      if (i == 0) {                              // a whole variant of the pattern occurs
        if (WRITE) { if (g == 0) fmx_mm_emit(sl, nint, s, e, (uint32_t)d, ed0, ed1, out_s, out_e, out_edit); }
        nint++;
        rows += e - s;
        d--;
      } else {
        // the symbol of this trip: the next candidate that occurs in the text, else the pattern's own
        uint32_t c = maxc + 1u;
        if ((uint32_t)d < K) {
          c = d == 0 ? fc0 : fc1;
          while (c <= maxc) {                    // lane g looks at symbol c + g
            const uint32_t cc = c + g;
            bool here = cc <= maxc && cc != p;
            if (here && ix.cs) here = (cc < maxc ? ix.cs[cc + 1] : ctot) != ix.cs[cc];
            const uint32_t nx = fmx_group_min(here ? cc : 0xFFFFFFFFu);
            if (nx != 0xFFFFFFFFu) { c = nx; break; }
            c += FMX_GROUP;
          }
          if (c > maxc) c = maxc + 1u;
        }
        const bool sub = c <= maxc;
        const uint32_t sym = sub ? c : p;
        if (sym <= maxc) {
          // the symbol in front of this one rides along with the record loads
          const uint32_t pn = i > 1 ? fmx_load_sym(pat, ix.sym_bytes, pbeg + i - 2) : 0u;
          uint32_t ns = s, ne = e;
          fmx_lf_map2_pair<KIND, NL, SM>(ix, sym, ns, ne, g);
          // (ne < ns: lf_map2(0, .) of a multi-pieces index is not monotone, multi_pieces.rs:147-153 -- no row)
          const bool hit = ne > ns;
          if (sub) {
            if (d == 0) fc0 = c + 1u; else fc1 = c + 1u;
            if (hit) {                           // descend: one more substitution spent
              const uint64_t ed = ((uint64_t)(i - 1u) << 32) | c;
              if (d == 0) { ed0 = ed; fi1 = i - 1u; fs1 = ns; fe1 = ne; fp1 = pn; fc1 = 1; }
              else { ed1 = ed; fi2 = i - 1u; fs2 = ns; fe2 = ne; fp2 = pn; }
              d++;
            }
          } else if (hit) {                      // the pattern's own symbol: the frame moves on, same level
            if (d == 0) { fi0 = i - 1u; fs0 = ns; fe0 = ne; fp0 = pn; fc0 = 1; }
            else if (d == 1) { fi1 = i - 1u; fs1 = ns; fe1 = ne; fp1 = pn; fc1 = 1; }
            else { fi2 = i - 1u; fs2 = ns; fe2 = ne; fp2 = pn; }
          } else {
            d--;
          }
        } else {
          d--;                                   // a symbol that is absent from the alphabet cannot match
        }
      }
    }
    if (d < 0) {
      if (g == 0) fmx_mm_finish<WRITE>(sl, k, total, nint, rows, ix.status, out_nint, out_cnt);
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// the index of an EMPTY text emits nothing; one lane per pattern, offsets and given ranges checked like everywhere
template <bool WRITE>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_mm_empty_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0,
    const uint64_t *__restrict__ out_off, uint64_t total, uint64_t *__restrict__ out_nint,
    uint64_t *__restrict__ out_cnt) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    const uint64_t a = off[k], b = off[k + 1];
    if (FMX_SPAN_BAD(a, b, pmin, ptot) || (s0e0 && (s0e0[2 * k] | s0e0[2 * k + 1]) != 0))
      atomicOr(status, 1u << FMX_ERR_ARG);
    FmxMmSlots sl{0, 0, 0};
    if (WRITE) sl = fmx_mm_slots(out_off, k, total);
    fmx_mm_finish<WRITE>(sl, k, total, 0, 0, status, out_nint, out_cnt);
  }
}

// single 3-bit level (DNA), taken under the condition of fmx_count_f3_kernel.  Lane g of a group holds the counter of
// code g and the three bit planes of its 32 rows, so after the two dwordx4 loads of a step the rank of EVERY symbol is
// register work.  A frame (level t < K) keeps its two pieces and a mask of the substitutions whose interval is not
// empty; each is followed to its end, then the frame is resumed: the next symbol of the mask is re-ranked from the
// kept pieces, no reload.  Level K is the plain exact step.  The symbol of a step is requested with its records.
struct FmxMmFrame { uint4 a, b; uint32_t i, s, e, p, mask; };
template <int K, bool WRITE>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_mm_f3_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, const uint64_t *__restrict__ out_off, uint64_t total,
    uint64_t *__restrict__ out_nint, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol

  uint64_t k = gid, pbeg = 0, nint = 0, rows = 0;
  bool active = k < npat, fresh = true;
  uint32_t i = 0, s = 0, e = 0;                  // the node to visit: i symbols still to prepend to (s, e)
  int d = 0;                                     // its level = substitutions spent
  int r = -1;                                    // frame to resume (-1: none, visit the node)
  bool fin = false;
  FmxMmFrame f[K > 0 ? K : 1];
  uint64_t ed[2] = {0, 0};
  FmxMmSlots sl{0, 0, 0};
  while (active) {
    if (fresh) {
      uint32_t m;
      nint = 0; rows = 0;
      if (WRITE) sl = fmx_mm_slots(out_off, k, total);
      fin = !fmx_mm_begin(off, s0e0, k, pmin, ptot, n, status, g, pbeg, m, s, e);
      i = m; d = 0; r = -1;
      fresh = false;
    }
    if (!fin) {
      // ---- visit (i, s, e) at level d ----
      if (i == 0) {                              // a whole variant of the pattern occurs
        if (WRITE) { if (g == 0) fmx_mm_emit(sl, nint, s, e, (uint32_t)d, ed[0], ed[1], out_s, out_e, out_edit); }
        nint++;
        rows += e - s;
        if (d == 0) fin = true; else r = d - 1;
      } else {
        const uint32_t rs = s >> 8, re = e >> 8;
        FMX_CHECK(rs < nrec && re < nrec);
        FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
        if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
        const uint4 a = rec[(size_t)rs * 8u + g];
        const uint4 b = rec[(size_t)re * 8u + g];
        const uint32_t p = pat[pbeg + i - 1u];   // requested with the records
        bool framed = false;
#pragma unroll
        for (int t = 0; t < K; t++) {
          if (d == t) {                          // a level with budget left: keep the pieces, rank every symbol
            uint32_t mask = 0;
#pragma unroll
            for (uint32_t c = 1; c < 8u; c++) {
              if (c <= max_character && c != p) {
                const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
                const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
                mask |= (uint32_t)(ne > ns) << c;
              }
            }
            f[t].a = a; f[t].b = b; f[t].i = i; f[t].s = s; f[t].e = e; f[t].p = p; f[t].mask = mask;
            r = t;
            framed = true;
          }
        }
        if (!framed) {                           // level K: the plain exact step
          bool hit = false;
          if (p <= max_character) {
            const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, p, g));
            const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, p, g));
            hit = ne > ns;
            if (hit) { s = ns; e = ne; i--; }
          }
          if (!hit) { if (d == 0) fin = true; else r = d - 1; }
        }
      }
      // ---- resume frames, innermost first: a frame that is used up hands over to the one below it ----
#pragma unroll
      for (int t = K - 1; t >= 0; t--) {
        if (!fin && r == t) {
          FmxMmFrame &F = f[t];
          const bool sub = F.mask != 0u;
          const uint32_t c = sub ? (uint32_t)__ffs((int)F.mask) - 1u : F.p;
          F.mask &= F.mask - 1u;
          bool hit = false;
          if (sub || c <= max_character) {
            const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(F.a, F.s & 255u, c, g));
            const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(F.b, F.e & 255u, c, g));
            hit = ne > ns;                       // (a substitution of the mask always is)
            if (hit) { s = ns; e = ne; i = F.i - 1u; }
          }
          if (hit) {
            if (sub) ed[t] = ((uint64_t)(F.i - 1u) << 32) | c;
            d = sub ? t + 1 : t;                 // the pattern's own symbol keeps the level: the frame is replaced
            r = -1;
          } else if (t == 0) {
            fin = true;
          } else {
            r = t - 1;
          }
        }
      }
    }
    if (fin) {
      if (g == 0) fmx_mm_finish<WRITE>(sl, k, total, nint, rows, status, out_nint, out_cnt);
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// ---- launch ----
struct FmxMmCall {
  const fmx_index *idx; FmxDev dv; const void *pat; const uint64_t *off; uint64_t npat; const uint64_t *s0e0;
  uint32_t K; const uint64_t *out_off; uint64_t total; uint64_t *nint, *cnt, *s, *e, *edit; hipStream_t st;
  unsigned grid;
};
// the ladder of fmx_route() (fmx_query.hip) without its accelerators and without the endpoint-per-lane shape: the
// one-level DNA kernel, else the group-per-pattern kernel of the index kind.  write = false: pass 1 (d_nint, d_cnt);
// write = true: pass 2 (d_out_off, total, d_s, d_e, d_edit).  The caller has refused K > FMX_MAX_MISMATCHES and
// handles of the wide engine.
template <bool WR>
static int fmx_launch_mismatch_pass(const FmxMmCall &c) {
  const dim3 grid(c.grid), block(FMX_BLOCK);
  if (c.idx->n == 0) {                               // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_mm_empty_kernel<WR>, dim3(fmx_grid_for_groups((c.npat + 7) / 8)), block, 0, c.st,
                       c.dv.status, c.off, c.npat, c.s0e0, c.out_off, c.total, c.nint, c.cnt);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  const FmxRoute r = fmx_route(c.idx, c.dv, fmx_tune(), FMX_SHAPE_F3 | FMX_SHAPE_GROUP);
  if (r.shape == FMX_SHAPE_F3) {
    auto f3 = [&](auto kk) {
      hipLaunchKernelGGL((fmx_mm_f3_kernel<kk(), WR>), grid, block, 0, c.st, c.dv.bw.lv[0].rec, c.dv.n,
                         c.dv.max_character, c.dv.status, (const uint8_t *)c.pat, c.off, c.npat, c.s0e0, c.out_off,
                         c.total, c.nint, c.cnt, c.s, c.e, c.edit);
    };
    if (c.K == 0) f3(FmxInt<0>{}); else if (c.K == 1) f3(FmxInt<1>{}); else f3(FmxInt<2>{});
  } else {
    fmx_route_group(r, [&](auto kind, auto nl, auto sm, auto) {
      hipLaunchKernelGGL((fmx_mm_kernel<kind(), nl(), sm(), WR>), grid, block, 0, c.st, c.dv, c.pat, c.off, c.npat,
                         c.s0e0, c.K, c.out_off, c.total, c.nint, c.cnt, c.s, c.e, c.edit);
    });
  }
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
int fmx_launch_mismatch(const fmx_index *idx, const void *d_pat, const uint64_t *d_off, uint64_t npat,
                        const uint64_t *d_s0e0, uint32_t max_mismatches, bool write, const uint64_t *d_out_off,
                        uint64_t total, uint64_t *d_nint, uint64_t *d_cnt, uint64_t *d_s, uint64_t *d_e,
                        uint64_t *d_edit, hipStream_t st) {
  if (idx->is_wide || max_mismatches > FMX_MAX_MISMATCHES) return FMX_ERR_ARG;   // (refused with a message by the ABI)
  const FmxDev dv = fmx_launch_dev(idx);
  if (npat == 0) return FMX_OK;
  const FmxMmCall c{idx, dv, d_pat, d_off, npat, d_s0e0, max_mismatches, d_out_off, total, d_nint, d_cnt,
                    d_s, d_e, d_edit, st, fmx_grid_for_groups(npat)};
  return write ? fmx_launch_mismatch_pass<true>(c) : fmx_launch_mismatch_pass<false>(c);
}
