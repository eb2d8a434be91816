// fmx_packed_mstats.h -- matching statistics and SMEM seeds on 2-bit packed DNA patterns, one strand or both
// (fmx_match_stats_batch_packed2* / fmx_match_stats_batch_packed2_rc*; included by fmx_query.hip after fmx_packed.h,
// fmx_packed_rc.h and fmx_mstats.h, whose layout, fmx_p2_* / fmx_p2rc_* helpers, route, empty-text kernel and seed
// kernel it uses).
//
// The results are those of fmx_match_stats_batch (fmx_mstats.h) on the unpacked bytes, symbol = code + 1: a SLOT per
// pattern symbol, the same three passes on one stream, the same step rules.  The both-strand call answers the virtual
// batch V[2k] = P_k, V[2k + 1] = R_k (R[t] = 5 - P[m - 1 - t]): pattern k owns the 2 m_k slots from 2 (off[k] - off[0]),
// strand 0 first.  What is new is the FRONT END of a slot:
//   * the OWNER WORD.  The pre-pass (fmx_p2ms_owner_kernel) leaves in out_len[slot], instead of the pattern id,
//       strand 0:  the end position i in the low 32 bits and FMX_P2MS_LASTI where i == m;
//       strand 1:  FMX_P2MS_RC | k (this strand reads forward from symbol m - i: it needs the pattern's end);
//     all-ones (the memset) is an unowned slot.  The end symbol of strand-0 slot t of the single-strand call is symbol
//     pat_off[0] + t whoever owns it, so that kernel reads no offset at all, and a group requests the owner word AND
//     both stream words of its NEXT slot under the steps of the current one: a slot starts with its window's words in
//     registers and goes straight to the table entry.  In the both-strand call the slot number gives a strand-0 slot
//     its end symbol only together with i (u = 2 t - i + 1), so the words are requested when the owner word is there.
//     Whatever the word holds, a kernel bounds its own reads: strand 0 clamps i to the symbols between pat_off[0] and
//     the end symbol and refuses an end symbol at or beyond pat_off[npat]; strand 1 re-checks the offsets of k as the
//     byte kernel does.  No word without a symbol of [pat_off[0], pat_off[npat]) is touched.
//   * the WINDOW: the at most 32 unread symbols before the end position (strand 0: backward funnel, reversed once for
//     the steps; strand 1: forward funnel, complemented once), fmx_packed.h / fmx_packed_rc.h.  No step loads a pattern
//     symbol.  The one-symbol kernel requests the next window in the step that consumes the window's last symbol, with
//     that step's record loads; the pair kernel re-cuts the window when fewer than two of its symbols are left (it
//     needs both symbols of a probe), one wait per 31 or 32 symbols.
//   * the K-MER CODE: a shift of the stream-order window on 2-bit tables, recoded in registers on 3-bit tables and on
//     alphabets of fewer than four symbols, where a code that is no symbol sends the slot to the stepwise start.
// Work split of the both-strand call: STRAND PER GROUP.  Groups stride over the 2 total virtual slots; the strand is
// what the owner word says, so the groups of a wave may differ in their front end and share the steps.
#pragma once

#define FMX_P2MS_LASTI (1ull << 32)   // owner word of a strand-0 slot: i == m
#define FMX_P2MS_RC (1ull << 62)      // owner word of a strand-1 slot: the pattern id in the bits below

// the offsets of every pattern checked once (FMX_ERR_ARG as in the count kernels); the owner word of every slot of a
// valid pattern, never at or above the slot count (total, or 2 total with both strands)
template <bool RC>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_p2ms_owner_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total, uint64_t *__restrict__ owner) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = off[npat], pmin = off[0];
  if (gid == 0 && g == 0 && (ptot < pmin || ptot - pmin != total)) atomicOr(status, 1u << FMX_ERR_ARG);
  const uint64_t nslot = RC ? 2u * total : total;
  for (uint64_t k = gid; k < npat; k += ngroups) {
    const uint64_t pbeg = off[k], pend = off[k + 1];
    if (FMX_SPAN_BAD32(pbeg, pend, pmin, ptot)) {
      if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      continue;
    }
    const uint64_t m = pend - pbeg, u0 = (RC ? 2u : 1u) * (pbeg - pmin);
    for (uint64_t x = g; x < (RC ? 2u * m : m) && u0 + x < nslot; x += FMX_GROUP)
      owner[u0 + x] = x < m ? (x + 1u) | (x + 1u == m ? FMX_P2MS_LASTI : 0ull) : FMX_P2MS_RC | k;
  }
}

// slot u with the owner word w: its strand, the stream position its window is cut from (`base`: the pattern's first
// symbol on strand 0, the symbol after its last on strand 1), its end position i and whether i == m.  false = unowned:
// nothing may be read for it.  span = pat_off[npat] - pat_off[0] (0 when that is negative).
template <bool RC>
__device__ __forceinline__ bool fmx_p2ms_slot(const uint64_t *__restrict__ off, uint64_t npat, uint64_t pmin,
                                              uint64_t ptot, uint64_t span, uint64_t u, uint64_t w, bool &rc,
                                              uint64_t &base, uint32_t &i, bool &last) {
  rc = false;
  if (w == ~0ull) return false;
  if (RC && (w & FMX_P2MS_RC)) {
    const uint64_t k = w & (FMX_P2MS_RC - 1u);
    if (k >= npat) return false;
    const uint64_t pbeg = off[k], pend = off[k + 1];
    if (FMX_SPAN_BAD32(pbeg, pend, pmin, ptot)) return false;
    const uint64_t m = pend - pbeg, u1 = 2u * (pbeg - pmin) + m;   // the strand's first slot
    if (u < u1 || u - u1 >= m) return false;
    i = (uint32_t)(u - u1) + 1u;
    last = i == m;
    base = pend;
    rc = true;
    return true;
  }
  i = (uint32_t)w;
  last = (w & FMX_P2MS_LASTI) != 0;
  uint64_t t = u;                                          // the slot of the end symbol in the stream: symbol pmin + t
  if (RC) {                                                // u = 2 t0 + i - 1, t = t0 + i - 1
    if (i == 0u || i > u + 1u || ((u + 1u - i) & 1u)) return false;
    t = ((u + 1u - i) >> 1) + i - 1u;
  } else if (i > t + 1u) {
    i = (uint32_t)(t + 1u);                                // never before pat_off[0]
  }
  if (t >= span) return false;
  base = pmin + t + 1u - i;
  return true;
}

// ---------------------------------------------------------------------------
// single 3-bit level (the twin of fmx_ms_f3_kernel): one symbol per step out of the window.  max_character may be
// below 4 in the single-strand call: a code that is no symbol of the index ends the match.  RC: the slots of both
// strands (max_character >= 4, the dispatcher's rule).  SGPRs capped like the packed count kernels': uncapped, three
// of the eight instantiations take 82 to 95 and would not start 8 waves per SIMD.
// ---------------------------------------------------------------------------
template <bool KM, bool RC>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_ms_f3_p2_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits,
    const uint64_t *__restrict__ words, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total,
    uint32_t mc, uint32_t cap, uint64_t lastbit, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t t = gid, base = 0, win = 0, lastw = 0;
  bool active = t < total, fresh = true, rc = false;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;   // j unread symbols of the prefix, jw of them not in `win`
  const uint64_t ptot = off[npat], pmin = off[0];
  const uint64_t span = ptot >= pmin ? ptot - pmin : 0;
  // the group's NEXT slot travels under the current slot's steps: its owner word and, on a single strand, the word of
  // its end symbol and the word of the symbol 31 before it (or of pat_off[0]) -- every window of the slot is cut of these
  uint64_t nw = 0, nhi = 0, nlo = 0;
  auto request = [&](uint64_t tn) {
    if (tn >= total) return;
    nw = out_len[tn];
    if (!RC && tn < span) {
      const uint64_t E = pmin + tn + 1u;
      nhi = words[(E - 1u) >> 5];
      nlo = words[(tn >= 32u ? E - 32u : pmin) >> 5];
    }
  };
  request(t);
  while (active) {
    if (fresh) {
      const uint64_t w = nw, hi = nhi, lo = nlo;
      request(t + ngroups);
      uint32_t i = 0;
      bool last = false;
      s = 0; e = n; len = 0; j = 0; jw = 0; lastw = 0;
      if (fmx_p2ms_slot<RC>(off, npat, pmin, ptot, span, t, w, rc, base, i, last)) {
        lastw = last ? lastbit : 0ull;
        if (n >= mc) j = i;                                // (a whole index below min_count: no step can pass)
        if (j) {
          const uint32_t cnt = j > 32u ? 32u : j;
          const uint64_t raw = RC ? fmx_p2rc_raw(words, rc, base, j, cnt) : fmx_p2_funnel(hi, lo, base + j);
          jw = j - cnt;
          win = fmx_p2rc_steps(raw, rc);
          if (KM && j >= kmer_k && cap >= kmer_k) {        // all kmer_k symbols at once when the entry is wide enough
            uint32_t code;
            bool ok = true;
            if (kmer_bits == 2u && max_character >= 4u) code = fmx_p2rc_code2(raw, rc, kmer_k);
            else ok = fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);
            if (ok) {
              FMX_TOUCH_G0N(g, &kmer[code]);
              const uint2 se = kmer[code];
              if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; win >>= 2u * kmer_k; }
            }
          }
        }
      }
      fresh = false;
    }
    const uint32_t c = ((uint32_t)win & 3u) + 1u;          // the symbol consumed next
    bool done = j == 0 || len >= cap || c > max_character; // an absent symbol ends the match
    if (!done) {
      const uint32_t rs = s >> 8, re = e >> 8;
      FMX_CHECK(rs < nrec && re < nrec);
      FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
      if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
      const uint4 a = rec[(size_t)rs * 8u + g];
      const uint4 b = rec[(size_t)re * 8u + g];
      // this step takes the window's last symbol and the prefix has more: the next window rides along
      const bool refill = j - jw == 1u && jw != 0u;
      const uint32_t cnt = jw > 32u ? 32u : jw;
      uint64_t raw = 0;
      if (refill) raw = fmx_p2rc_raw(words, RC && rc, base, jw, cnt);
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
      if (ne - ns < mc) {
        done = true;                                       // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        j--;
        win >>= 2u;
        if (refill) { win = fmx_p2rc_steps(raw, RC && rc); jw -= cnt; }
        done = j == 0;
      }
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[t] = len ? s : 0u;
        if (out_e) out_e[t] = len ? e : 0u;
        out_len[t] = (uint64_t)len | lastw;
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
}

// ---------------------------------------------------------------------------
// the pair index (the twin of fmx_ms_pair_kernel; max_character == 4 and 2-bit table codes, the dispatcher's rule, so
// every code is a symbol of the index and `win & 15` is the pair record's code).  The step rules are that kernel's:
// a pair probe while two symbols remain and the cap leaves room for two, taken when it keeps >= min_count rows;
// otherwise the single step for the last symbol, after which a failed pair probe ends the match; no pair probe with
// one symbol of budget left; the code-0 row correction.
// ---------------------------------------------------------------------------
template <bool KM, bool RC>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_ms_pair_p2_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    const uint2 *__restrict__ kmer, uint32_t kmer_k,
    const uint64_t *__restrict__ words, const uint64_t *__restrict__ off, uint64_t npat, uint64_t total,
    uint32_t mc, uint32_t cap, uint64_t lastbit, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t t = gid, base = 0, win = 0, lastw = 0;
  bool active = t < total, fresh = true, rc = false;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;   // j unread symbols of the prefix, jw of them not in `win`
  const uint64_t ptot = off[npat], pmin = off[0];
  const uint64_t span = ptot >= pmin ? ptot - pmin : 0;
  uint64_t nw = 0, nhi = 0, nlo = 0;               // the group's next slot: see fmx_ms_f3_p2_kernel
  auto request = [&](uint64_t tn) {
    if (tn >= total) return;
    nw = out_len[tn];
    if (!RC && tn < span) {
      const uint64_t E = pmin + tn + 1u;
      nhi = words[(E - 1u) >> 5];
      nlo = words[(tn >= 32u ? E - 32u : pmin) >> 5];
    }
  };
  request(t);
  while (active) {
    if (fresh) {
      const uint64_t w = nw, hi = nhi, lo = nlo;
      request(t + ngroups);
      uint32_t i = 0;
      bool last = false;
      s = 0; e = n; len = 0; j = 0; jw = 0; lastw = 0;
      if (fmx_p2ms_slot<RC>(off, npat, pmin, ptot, span, t, w, rc, base, i, last)) {
        lastw = last ? lastbit : 0ull;
        if (n >= mc) j = i;                                // (a whole index below min_count: no step can pass)
        if (j) {
          const uint32_t cnt = j > 32u ? 32u : j;
          const uint64_t raw = RC ? fmx_p2rc_raw(words, rc, base, j, cnt) : fmx_p2_funnel(hi, lo, base + j);
          jw = j - cnt;
          win = fmx_p2rc_steps(raw, rc);
          if (KM && j >= kmer_k && cap >= kmer_k) {        // all kmer_k symbols at once when the entry is wide enough
            const uint32_t code = fmx_p2rc_code2(raw, rc, kmer_k);
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; win >>= 2u * kmer_k; }
          }
        }
      }
      fresh = false;
    }
    bool done = j == 0 || len >= cap;
    if (!done) {
      if (j - jw < 2u && jw != 0u) {                       // a probe needs two symbols: re-cut the window at the unread end
        const uint32_t cnt = j > 32u ? 32u : j;
        const uint64_t raw = fmx_p2rc_raw(words, RC && rc, base, j, cnt);
        jw = j - cnt;
        win = fmx_p2rc_steps(raw, RC && rc);
      }
      const uint32_t code = (uint32_t)win & 15u;           // (c1 - 1) * 4 + (c2 - 1): c2 the symbol consumed first
      const uint32_t c2 = (code & 3u) + 1u;
      const bool pair = j - jw >= 2u && cap - len >= 2u;
      uint32_t used = 0;
      if (pair) {
        FMX_CHECK((s >> 7) < n / 128u + 1u && (e >> 7) < n / 128u + 1u);
        FMX_TOUCH_G0(g, &rec2[(size_t)(s >> 7) * 8u]);
        if ((e >> 7) != (s >> 7)) FMX_TOUCH_G0(g, &rec2[(size_t)(e >> 7) * 8u]);
        const uint4 a = rec2[(size_t)(s >> 7) * 8u + g];
        const uint4 b = rec2[(size_t)(e >> 7) * 8u + g];
        uint32_t ns = fmx_group_sum(fmx_piece_rank<4>(a, s & 127u, code, g));
        uint32_t ne = fmx_group_sum(fmx_piece_rank<4>(b, e & 127u, code, g));
        if (code == 0u) {  // the two rows without a 2-gram are stored as code 0
          ns -= (uint32_t)(s > row0) + (uint32_t)(s > row1);
          ne -= (uint32_t)(e > row0) + (uint32_t)(e > row1);
        }
        if (ne - ns >= mc) { s = ns; e = ne; used = 2; }
      }
      if (used == 0) {       // one symbol on the 1-gram records
        FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
        FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
        const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
        const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
        const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));
        const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));
        if (e1 - s1 >= mc) { s = s1; e = e1; used = 1; }
        done = pair || used == 0;                          // after a failed pair probe the second symbol is known to fail
      }
      len += used;
      j -= used;
      win >>= 2u * used;
      done |= j == 0;
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[t] = len ? s : 0u;
        if (out_e) out_e[t] = len ? e : 0u;
        out_len[t] = (uint64_t)len | lastw;
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
}

// ---- launch: fmx_packed2_route()'s two rungs and the empty text.  The caller has refused a handle the route does not
// serve (fmx_packed2_served / fmx_packed2_rc_served) and a NULL d_len; npat > 0.  `total` is the span of the offsets,
// the arrays have total entries, or 2 total with both strands. ----
int fmx_launch_match_stats_packed2(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                                   uint64_t total, uint64_t min_count, uint64_t max_len, uint64_t min_seed_len,
                                   uint64_t *d_s, uint64_t *d_e, uint64_t *d_len, bool both, hipStream_t st) {
  if (min_count == 0) min_count = 1;
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  const uint64_t nslot = both ? 2u * total : total;
  const bool seeds = min_seed_len > 0 && (d_s || d_e);
  if (nslot) FMX_HIP(hipMemsetAsync(d_len, 0xFF, (size_t)nslot * 8, st));
  if (both)
    hipLaunchKernelGGL(fmx_p2ms_owner_kernel<true>, dim3(fmx_grid_for_groups(npat)), dim3(FMX_BLOCK), 0, st, dv.status,
                       d_off, npat, total, d_len);
  else
    hipLaunchKernelGGL(fmx_p2ms_owner_kernel<false>, dim3(fmx_grid_for_groups(npat)), dim3(FMX_BLOCK), 0, st, dv.status,
                       d_off, npat, total, d_len);
  FMX_HIP(hipGetLastError());
  if (nslot == 0) return FMX_OK;                     // (the owner pass has compared the offsets with it)
  if (idx->n == 0) {                                 // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_ms_empty_kernel, dim3(fmx_grid_for_groups((nslot + 7) / 8)), dim3(FMX_BLOCK), 0, st, nslot,
                       d_s, d_e, d_len);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  const uint32_t mc = min_count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)min_count;
  const uint32_t cap = (max_len == 0 || max_len > 0xFFFFFFFFull) ? 0xFFFFFFFFu : (uint32_t)max_len;
  const uint64_t lastbit = seeds ? FMX_MS_LAST : 0ull;
  const dim3 grid(fmx_grid_for_groups(nslot)), block(FMX_BLOCK);
  auto strands = [&](auto f) { if (both) f(std::true_type{}); else f(std::false_type{}); };
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      strands([&](auto rc) {
        hipLaunchKernelGGL((fmx_ms_pair_p2_kernel<decltype(km)::value, decltype(rc)::value>), grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                           dv.pair_row0, dv.pair_row1, dv.kmer, dv.kmer_k, d_words, d_off, npat, nslot, mc, cap, lastbit,
                           d_s, d_e, d_len);
      });
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      strands([&](auto rc) {
        hipLaunchKernelGGL((fmx_ms_f3_p2_kernel<decltype(km)::value, decltype(rc)::value>), grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character,
                           dv.kmer, dv.kmer_k, dv.kmer_bits, d_words, d_off, npat, nslot, mc, cap, lastbit, d_s, d_e,
                           d_len);
      });
    });
  }
  FMX_HIP(hipGetLastError());
  if (seeds) {
    hipLaunchKernelGGL(fmx_ms_seed_kernel, dim3(fmx_grid_for_groups((nslot + 7) / 8)), dim3(FMX_BLOCK), 0, st, nslot,
                       min_seed_len, d_s, d_e, d_len);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}
