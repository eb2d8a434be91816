// fmx_packed_mismatch.h -- backward search with up to FMX_MAX_MISMATCHES substitutions on 2-bit packed DNA patterns, one
// strand or both, in ONE pass into caller-sized slots (fmx_mismatch_hits_batch_packed2* / ..._rc*; included by
// fmx_query.hip after fmx_packed.h, fmx_packed_rc.h and fmx_mismatch.h, whose layout, fmx_p2_* / fmx_p2rc_* helpers and
// route it uses).
//
// The enumeration and its order are those of fmx_mismatch.h, run from (0, len) on the symbols of the virtual pattern
// v: v = k on a single strand; v = 2 k + strand on both, strand 1 the reverse complement R[t] = 5 - P[m - 1 - t].
// Kept from fmx_mm_f3_kernel: the 8-lane group per pattern, lane g holding counter g and the three bit planes of its 32
// rows (every symbol of a position is ranked from the two dwordx4 loads of a step), the flat loop with at most one pair
// of record requests per trip, the K named frames with their kept pieces and substitution mask.  What is new:
//   * the WINDOW.  The next <= 32 symbols to consume are one 64-bit value in steps order (fmx_packed_rc.h): a step
//     reads `win & 3` and shifts; `i` counts the unread symbols, `jw` those of them that are not in the window.  Strand 0
//     cuts it from the pattern's end and reverses the fields, strand 1 cuts it forward from the pattern's start and
//     complements it once per fill.  No step loads a pattern symbol; the window that follows is requested in the step
//     that consumes the window's last symbol, together with that step's two record loads.
//   * FRAMES KEEP THEIR CHILDREN'S WINDOW.  Every child of a node -- each substitution and the pattern's own symbol --
//     continues with the same window: the node's shifted by one symbol, or the refill the node's step requested.  A
//     frame saves that window and its `jw` next to the pieces, so resuming it returns the search to an earlier position,
//     also one on the other side of a refill, without a load and without a wait.  The frame's own symbol travels in
//     bits 8..10 of its mask word.  Per frame that is 15 registers against the byte kernel's 13.
//   * STRAND PER WAVE (RC): the waves of a block alternate strands over the same eight patterns (fmx_p2rc_split), so
//     the front-end choice is a scalar branch.
//   * ONE PASS.  Virtual pattern v owns slots [v max_hits, (v + 1) max_hits): lane 0 writes interval j there while
//     j < max_hits and the search keeps COUNTING beyond that, so nint and count are exact; at the pattern's end the
//     lanes of the group fill the unused slots (s = e = 0, edits all-ones) and lane 0 stores nint and count.  No offsets
//     array is read, nothing is walked twice.
// The pattern start is not prefetched under the previous pattern's steps (the packed pair kernel's pipeline): its two
// deep state would be live across every frame.  No LDS, no scratch.
#pragma once

// interval number j of virtual pattern v; d substitutions were made (lane 0 of the group)
__device__ __forceinline__ void fmx_p2mm_emit(uint64_t v, uint64_t max_hits, uint64_t j, uint32_t s, uint32_t e, int d,
                                              uint64_t ed0, uint64_t ed1, uint64_t *__restrict__ out_s,
                                              uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  if (j < max_hits) {
    const uint64_t slot = v * max_hits + j;
    if (out_s) out_s[slot] = s;
    if (out_e) out_e[slot] = e;
    if (out_edit) {
      out_edit[2 * slot] = d > 0 ? ed0 : ~0ull;
      out_edit[2 * slot + 1] = d > 1 ? ed1 : ~0ull;
    }
  }
}
// end of virtual pattern v: lanes g, g + stride, ... fill the slots no interval took; lane 0 stores the totals
__device__ __forceinline__ void fmx_p2mm_finish(uint64_t v, uint64_t max_hits, uint64_t nint, uint64_t rows, uint32_t g,
                                                uint32_t stride, uint64_t *__restrict__ out_nint,
                                                uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_s,
                                                uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  for (uint64_t j = (nint < max_hits ? nint : max_hits) + g; j < max_hits; j += stride) {
    const uint64_t slot = v * max_hits + j;
    if (out_s) out_s[slot] = 0;
    if (out_e) out_e[slot] = 0;
    if (out_edit) { out_edit[2 * slot] = ~0ull; out_edit[2 * slot + 1] = ~0ull; }
  }
  if (g == 0) {
    if (out_nint) out_nint[v] = nint;
    if (out_cnt) out_cnt[v] = rows;
  }
}

// a level with budget left: the two pieces of its node, the node itself, the window its children continue with, and
// mp = the substitutions whose interval is not empty (bits 1..7) | the node's own symbol << 8
struct FmxP2mmFrame { uint4 a, b; uint64_t win; uint32_t i, s, e, jw, mp; };

template <int K, bool RC>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_mm_f3_p2_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint64_t *__restrict__ words, const uint64_t *__restrict__ off, uint64_t npat, uint64_t max_hits,
    uint64_t *__restrict__ out_nint, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  bool rc = false;
  if (RC) {
    rc = fmx_p2rc_split(gid, ngroups);
  } else {
    gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
    ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  }
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)

  uint64_t k = gid, base = 0, win = 0, nint = 0, rows = 0;
  bool active = k < npat, fresh = true;
  uint32_t i = 0, jw = 0, s = 0, e = 0;          // the node to visit: i symbols still to prepend to (s, e), jw of them not in `win`
  int d = 0;                                     // its level = substitutions spent
  int r = -1;                                    // frame to resume (-1: none, visit the node)
  bool fin = false;
  FmxP2mmFrame f[K > 0 ? K : 1];
  uint64_t ed[2] = {0, 0};
  while (active) {
    if (fresh) {
      const uint64_t pbeg = off[k], pend = off[k + 1];
      // offsets that go backwards or leave the pattern stream: refuse, do not read
      fin = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      if (fin && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      base = rc ? pend : pbeg;                   // the window's edge is base + unread on strand 0, base - unread on strand 1
      nint = 0; rows = 0;
      s = 0; e = n;                              // (0, len): holds a row, n > 0 here
      i = fin ? 0u : (uint32_t)(pend - pbeg);
      jw = i; d = 0; r = -1;
      if (i) {
        const uint32_t cnt = i > 32u ? 32u : i;
        win = fmx_p2rc_steps(fmx_p2rc_raw(words, rc, base, i, cnt), rc);
        jw = i - cnt;
      }
      fresh = false;
    }
    if (!fin) {
      // ---- visit (i, s, e) at level d ----
      if (i == 0) {                              // a whole variant of the pattern occurs
        if (g == 0) fmx_p2mm_emit((RC ? 2u * k + (rc ? 1u : 0u) : k), max_hits, nint, s, e, d, ed[0], ed[1], out_s, out_e, out_edit);
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
        // this step takes the window's last symbol and the pattern has more: the next window rides along
        const bool refill = i - jw == 1u && jw != 0u;
        const uint32_t cnt = jw > 32u ? 32u : jw;
        uint64_t raw = 0;
        if (refill) raw = fmx_p2rc_raw(words, rc, base, jw, cnt);
        const uint32_t p = ((uint32_t)win & 3u) + 1u;
        // what every child of this node continues with
        const uint64_t cwin = refill ? fmx_p2rc_steps(raw, rc) : win >> 2;
        const uint32_t cjw = refill ? jw - cnt : jw;
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
            f[t].a = a; f[t].b = b; f[t].win = cwin; f[t].i = i; f[t].s = s; f[t].e = e; f[t].jw = cjw;
            f[t].mp = mask | (p << 8);
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
            if (hit) { s = ns; e = ne; i--; win = cwin; jw = cjw; }
          }
          if (!hit) { if (d == 0) fin = true; else r = d - 1; }
        }
      }
      // ---- resume frames, innermost first: a frame that is used up hands over to the one below it ----
#pragma unroll
      for (int t = K - 1; t >= 0; t--) {
        if (!fin && r == t) {
          FmxP2mmFrame &F = f[t];
          const bool sub = (F.mp & 0xFFu) != 0u;
          const uint32_t c = sub ? (uint32_t)__ffs((int)F.mp) - 1u : F.mp >> 8;
          if (sub) F.mp &= F.mp - 1u;
          bool hit = false;
          if (sub || c <= max_character) {
            const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(F.a, F.s & 255u, c, g));
            const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(F.b, F.e & 255u, c, g));
            hit = ne > ns;                       // (a substitution of the mask always is)
            if (hit) { s = ns; e = ne; i = F.i - 1u; win = F.win; jw = F.jw; }
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
      fmx_p2mm_finish((RC ? 2u * k + (rc ? 1u : 0u) : k), max_hits, nint, rows, g, FMX_GROUP, out_nint, out_cnt, out_s,
                      out_e, out_edit);
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// the index of an EMPTY text emits nothing: the offsets are still checked, every slot of every strand holds the filler.
// One lane per pattern, no word is read.
__global__ __launch_bounds__(FMX_BLOCK) void fmx_mm_empty_p2_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, uint32_t strands, uint64_t max_hits,
    uint64_t *__restrict__ out_nint, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_edit) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    if (FMX_SPAN_BAD(off[k], off[k + 1], pmin, ptot)) atomicOr(status, 1u << FMX_ERR_ARG);
    for (uint64_t v = strands * k; v < strands * k + strands; v++)
      fmx_p2mm_finish(v, max_hits, 0, 0, 0, 1, out_nint, out_cnt, out_s, out_e, out_edit);
  }
}

// ---- launch.  Indexes with the pair index or the k-mer table are served from their plain records, as in
// fmx_mismatch.h.  The caller has refused a handle the route does not serve (fmx_packed2_served / fmx_packed2_rc_served),
// max_mismatches > FMX_MAX_MISMATCHES and a slot count that does not fit 64 bits; npat > 0. ----
int fmx_launch_mismatch_hits_packed2(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                                     uint32_t max_mismatches, uint64_t max_hits, uint64_t *d_nint, uint64_t *d_cnt,
                                     uint64_t *d_s, uint64_t *d_e, uint64_t *d_edit, bool both, hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const dim3 block(FMX_BLOCK);
  if (idx->n == 0) {                                 // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_mm_empty_p2_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), block, 0, st, dv.status, d_off,
                       npat, both ? 2u : 1u, max_hits, d_nint, d_cnt, d_s, d_e, d_edit);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  const dim3 grid(fmx_grid_for_groups(both ? 2u * npat : npat));   // a group per strand of a pattern
  auto go = [&](auto kk, auto rc) {
    hipLaunchKernelGGL((fmx_mm_f3_p2_kernel<decltype(kk)::value, decltype(rc)::value>), grid, block, 0, st,
                       dv.bw.lv[0].rec, dv.n, dv.max_character, dv.status, d_words, d_off, npat, max_hits, d_nint, d_cnt,
                       d_s, d_e, d_edit);
  };
  auto strands = [&](auto kk) { if (both) go(kk, std::true_type{}); else go(kk, std::false_type{}); };
  if (max_mismatches == 0) strands(FmxInt<0>{}); else if (max_mismatches == 1) strands(FmxInt<1>{}); else strands(FmxInt<2>{});
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
