// fmx_packed_suffix.h -- longest-suffix match on 2-bit packed DNA patterns, one strand or both
// (fmx_suffix_match_batch_packed2*; included by fmx_query.hip after fmx_packed_rc.h, whose fmx_p2_* / fmx_p2rc_*
// helpers, strand split and route it uses).
//
// The STEP RULES are fmx_suffix.h's (a step is taken only while the stepped interval keeps >= mc rows, a table entry or
// a pair probe below mc says nothing about where the match stopped, a failed pair probe followed by one single step
// ends the match whatever that step gives); the FRONT ENDS are fmx_packed.h's and fmx_packed_rc.h's (the unread end of
// a pattern, up to 32 symbols, in one 64-bit steps window: `win & 3` the symbol to consume next, `win & 15` the pair
// record's code, a step shifts right; `j` counts the unread symbols, `jw` those of them that are not in the window).
// Four kernels, 8-lane groups, one 128-byte record line per lane, the group state machine of their byte twins:
//   fmx_sfx_pair_p2_kernel    max_character == 4 and 2-bit table codes, pair index; two-deep start pipeline
//   fmx_sfx_f3_p2_kernel      every other served handle (alphabets of 2 .. 7 symbols, 3-bit table codes); one symbol
//                             per step, the next window rides along with the record loads of the step that consumes
//                             the current one's last symbol
//   fmx_sfx_pair_p2rc_kernel  / fmx_sfx_f3_p2rc_kernel: both strands, strand per wave (fmx_p2rc_split), results to
//                             slots 2 k + strand
// What differs from the packed COUNT kernels, besides the rule and the fourth output: the table entry is CONDITIONAL
// (taken when it keeps >= mc rows; otherwise the window stays unshifted and the pattern steps from (0, n)), a start
// pair below mc ends a pattern before any of its words is requested, and a code that is no symbol of the index ends
// the match instead of raising FMX_ERR_SYMBOL_RANGE.  A suffix match ends early on most reads, so the start of a
// pattern is a larger share of its life than in count: the pair kernels start a pattern with its offsets admitted and
// its first word in a register.
// `mc` is min_count clamped to 1 .. 2^32 - 1 by the launcher, as in fmx_suffix.h.
#pragma once

// ---------------------------------------------------------------------------
// pair index, one strand (the twin of fmx_sfx_pair_kernel on the front end of fmx_count_pair_p2_kernel).  Every code
// is a symbol of the index, so the byte kernel's `pair` predicate is "two symbols are in the window": the refill keeps
// two there whenever the pattern has two.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_sfx_pair_p2_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    uint32_t *status, const uint2 *__restrict__ kmer, uint32_t kmer_k, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0, uint32_t mc,
    uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt,
    uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t k = gid;
  bool active = k < npat, fresh = true;
  uint64_t pbeg = 0, win = 0, hi = 0;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;
  bool badoff = false;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  typedef uint64_t fmx_u64x2 __attribute__((ext_vector_type(2), aligned(8)));
  fmx_u64x2 noff = {0, 0};
  uint64_t nbeg = 0, nhi = 0;
  uint32_t nj = 0;
  bool nbad = false;
  // noff (arrived; `live`: it belongs to a pattern) becomes the next pattern: its offsets are checked before anything
  // of it is read, its first word and the offsets of pattern `kn` are requested.  (With start pairs the word is not
  // prefetched: a pattern whose pair is refused or below mc is never read.)
  auto admit = [&](bool live, uint64_t kn) {
    nbeg = noff.x;
    const uint64_t pend = noff.y;
    nbad = live && FMX_SPAN_BAD32(nbeg, pend, pmin, ptot);
    nj = (nbad || !live) ? 0u : (uint32_t)(pend - nbeg);
    if (nj && !s0e0 && n >= mc) nhi = words[fmx_p2_word_hi(pend)];
    if (kn < npat) noff = *(const fmx_u64x2 *)(off + kn);
  };
  auto advance = [&]() { pbeg = nbeg; j = nj; badoff = nbad; hi = nhi; };
  if (active) noff = *(const fmx_u64x2 *)(off + k);
  admit(active, k + ngroups);
  advance();
  admit(k + ngroups < npat, k + 2u * ngroups);
  while (active) {
    if (fresh) {
      if (badoff && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      len = 0;
      if (s0e0) {
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        if (s64 > n || e64 > n || badoff) {            // not a range of this index: refuse, do not read
          if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
          s = 0; e = 0; j = 0;
        } else if (e < s || e - s < mc) {              // a start pair below min_count: no step can pass
          j = 0;
        }
        if (j) hi = words[fmx_p2_word_hi(pbeg + j)];
      } else {
        s = 0;
        e = badoff ? 0u : n;
        if (n < mc) j = 0;
      }
      jw = j;                                          // no window yet
    }
    // (re)fill the window: at the start of a pattern (its word is here already) and whenever fewer than two of its
    // symbols are left while the pattern has more -- one wait per 32 symbols
    if (j - jw < 2u && jw != 0u) {
      const uint64_t E = pbeg + j;
      const uint32_t cnt = j > 32u ? 32u : j;
      if (!fresh) hi = words[fmx_p2_word_hi(E)];
      uint64_t lo = 0;
      if (fmx_p2_straddles(E, cnt)) lo = words[(E - cnt) >> 5];
      const uint64_t str = fmx_p2_funnel(hi, lo, E);
      jw = j - cnt;
      win = fmx_p2_reverse(str);
      if (KM && fresh && !s0e0 && j >= kmer_k) {       // all kmer_k symbols at once when the entry is wide enough
        const uint32_t code = (uint32_t)(str >> (64u - 2u * kmer_k));
        FMX_TOUCH_G0N(g, &kmer[code]);
        const uint2 se = kmer[code];
        if (se.y - se.x >= mc) {
          s = se.x; e = se.y;
          j -= kmer_k; len = kmer_k;
          win >>= 2u * kmer_k;
        }
      }
    }
    fresh = false;
    bool done = (j == 0);
    if (!done) {
      const uint32_t code = (uint32_t)win & 15u;       // (c1 - 1) * 4 + (c2 - 1): c2 the last unread symbol
      const bool pair = j - jw >= 2u;
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
        const uint32_t c2 = (code & 3u) + 1u;
        FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
        FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
        const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
        const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
        const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));
        const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));
        if (e1 - s1 >= mc) { s = s1; e = e1; used = 1; }
        done = pair || used == 0;                      // after a failed pair probe the second symbol is known to fail
      }
      len += used;
      j -= used;
      win >>= 2u * used;
      done |= j == 0;
    }
    if (done) {
      // the pipeline moves on BEFORE the result stores are issued (see fmx_count_pair_kernel: loads and stores share
      // one counter, and only the next pattern's word and the offsets behind it are in flight here)
      __builtin_amdgcn_s_waitcnt(0x0F70);
      const uint64_t kd = k;
      advance();
      admit(k + 2u * ngroups < npat, k + 3u * ngroups);
      if (g == 0) {
        if (out_s) out_s[kd] = s;
        if (out_e) out_e[kd] = e;
        if (out_cnt) out_cnt[kd] = e >= s ? (uint64_t)(e - s) : 0ull;   // (a given start pair with e < s holds no row)
        if (out_len) out_len[kd] = len;
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// ---------------------------------------------------------------------------
// single 3-bit level, one strand (the twin of fmx_sfx_f3_kernel on the front end of fmx_count_f3_p2_kernel).
// max_character may be below 4 here: a code that is no symbol of the index ends the match when it is reached, and a
// table window that holds one skips the table.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_sfx_f3_p2_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0, uint32_t mc,
    uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt,
    uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t k = gid, pbeg = 0, win = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      // offsets that go backwards or leave the pattern stream: refuse, do not read (j = 0 from here on)
      bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      j = bad ? 0u : (uint32_t)(pend - pbeg);
      s = 0; e = n; len = 0;
      if (s0e0) {
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        bad |= s64 > n || e64 > n;                       // not a range of this index
      }
      if (bad) {
        if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
        s = 0; e = 0; j = 0;
      } else if (e < s || e - s < mc) {                  // a start pair below min_count: no step can pass
        j = 0;
      }
      jw = j;
      if (j) {
        const uint32_t cnt = j > 32u ? 32u : j;
        const uint64_t str = fmx_p2_load_window(words, pbeg + j, cnt);
        jw = j - cnt;
        win = fmx_p2_reverse(str);
        if (KM && !s0e0 && j >= kmer_k) {                // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          bool ok = true;
          if (kmer_bits == 2u && max_character >= 4u) code = (uint32_t)(str >> (64u - 2u * kmer_k));
          else ok = fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);
          if (ok) {
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            if (se.y - se.x >= mc) {
              s = se.x; e = se.y;
              j -= kmer_k; len = kmer_k;
              win >>= 2u * kmer_k;
            }
          }
        }
      }
      fresh = false;
    }
    const uint32_t c = ((uint32_t)win & 3u) + 1u;        // last unread symbol
    bool done = j == 0 || c > max_character;             // an absent symbol ends the match
    if (!done) {
      const uint32_t rs = s >> 8, re = e >> 8;
      FMX_CHECK(rs < nrec && re < nrec);
      FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
      if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
      const uint4 a = rec[(size_t)rs * 8u + g];
      const uint4 b = rec[(size_t)re * 8u + g];
      // this step takes the window's last symbol and the pattern has more: the next window rides along
      const bool refill = j - jw == 1u && jw != 0u;
      const uint32_t cnt = jw > 32u ? 32u : jw;
      uint64_t str = 0;
      if (refill) str = fmx_p2_load_window(words, pbeg + jw, cnt);
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
      if (ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        j--;
        win >>= 2u;
        if (refill) { win = fmx_p2_reverse(str); jw -= cnt; }
        done = j == 0;
      }
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[k] = s;
        if (out_e) out_e[k] = e;
        if (out_cnt) out_cnt[k] = e >= s ? (uint64_t)(e - s) : 0ull;   // (a given start pair with e < s holds no row)
        if (out_len) out_len[k] = len;
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// ---------------------------------------------------------------------------
// pair index, both strands (the twin of fmx_sfx_pair_p2_kernel on the front end of fmx_count_pair_p2rc_kernel): waves
// 2 p and 2 p + 1 serve the same eight patterns on opposite strands; `base` is pbeg on strand 0 and pend on strand 1,
// the first word in flight is word (pend - 1) / 32 there and word pbeg / 32 here.  No start pairs.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_sfx_pair_p2rc_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    uint32_t *status, const uint2 *__restrict__ kmer, uint32_t kmer_k, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, uint32_t mc, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2rc_split(gid, ngroups);

  uint64_t k = gid;
  bool active = k < npat, fresh = true;
  uint64_t base = 0, win = 0, w0 = 0;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;
  bool badoff = false;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  typedef uint64_t fmx_u64x2 __attribute__((ext_vector_type(2), aligned(8)));
  fmx_u64x2 noff = {0, 0};
  uint64_t nbase = 0, nw0 = 0;
  uint32_t nj = 0;
  bool nbad = false;
  // noff (arrived; `live`: it belongs to a pattern) becomes the next pattern: its offsets are checked before anything
  // of it is read, its first word and the offsets of pattern `kn` are requested
  auto admit = [&](bool live, uint64_t kn) {
    const uint64_t pbeg = noff.x, pend = noff.y;
    nbad = live && FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
    nj = (nbad || !live || n < mc) ? 0u : (uint32_t)(pend - pbeg);   // (0, n) below min_count: no step can pass
    nbase = rc ? pend : pbeg;
    if (nj) nw0 = words[rc ? pbeg >> 5 : fmx_p2_word_hi(pend)];
    if (kn < npat) noff = *(const fmx_u64x2 *)(off + kn);
  };
  auto advance = [&]() { base = nbase; j = nj; badoff = nbad; w0 = nw0; };
  if (active) noff = *(const fmx_u64x2 *)(off + k);
  admit(active, k + ngroups);
  advance();
  admit(k + ngroups < npat, k + 2u * ngroups);
  while (active) {
    if (fresh) {
      if (badoff && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      s = 0;
      e = badoff ? 0u : n;
      len = 0;
      jw = j;                                          // no window yet
    }
    // (re)fill the window: at the start of a pattern (its first word is here already) and whenever fewer than two of
    // its symbols are left while the pattern has more -- one wait per 32 symbols
    if (j - jw < 2u && jw != 0u) {
      const uint32_t cnt = j > 32u ? 32u : j;
      uint64_t raw;
      if (rc) {
        const uint64_t B = base - j;
        if (!fresh) w0 = words[B >> 5];
        uint64_t w1 = 0;
        if (fmx_p2_straddles_fwd(B, cnt)) w1 = words[(B >> 5) + 1u];
        raw = fmx_p2_funnel_fwd(w0, w1, B);
      } else {
        const uint64_t E = base + j;
        if (!fresh) w0 = words[fmx_p2_word_hi(E)];
        uint64_t w1 = 0;
        if (fmx_p2_straddles(E, cnt)) w1 = words[(E - cnt) >> 5];
        raw = fmx_p2_funnel(w0, w1, E);
      }
      jw = j - cnt;
      win = fmx_p2rc_steps(raw, rc);
      if (KM && fresh && j >= kmer_k) {                // all kmer_k symbols at once when the entry is wide enough
        const uint32_t code = fmx_p2rc_code2(raw, rc, kmer_k);
        FMX_TOUCH_G0N(g, &kmer[code]);
        const uint2 se = kmer[code];
        if (se.y - se.x >= mc) {
          s = se.x; e = se.y;
          j -= kmer_k; len = kmer_k;
          win >>= 2u * kmer_k;
        }
      }
    }
    fresh = false;
    bool done = (j == 0);
    if (!done) {
      const uint32_t code = (uint32_t)win & 15u;       // (c1 - 1) * 4 + (c2 - 1): c2 the symbol consumed first
      const bool pair = j - jw >= 2u;
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
        const uint32_t c2 = (code & 3u) + 1u;
        FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
        FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
        const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
        const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
        const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));
        const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));
        if (e1 - s1 >= mc) { s = s1; e = e1; used = 1; }
        done = pair || used == 0;                      // after a failed pair probe the second symbol is known to fail
      }
      len += used;
      j -= used;
      win >>= 2u * used;
      done |= j == 0;
    }
    if (done) {
      // the pipeline moves on BEFORE the result stores are issued (see fmx_count_pair_kernel: loads and stores share
      // one counter, and only the next pattern's word and the offsets behind it are in flight here)
      __builtin_amdgcn_s_waitcnt(0x0F70);
      const uint64_t v = 2u * k + (rc ? 1u : 0u);      // slot 2 k: the pattern; 2 k + 1: its reverse complement
      advance();
      admit(k + 2u * ngroups < npat, k + 3u * ngroups);
      if (g == 0) {
        if (out_s) out_s[v] = s;
        if (out_e) out_e[v] = e;
        if (out_cnt) out_cnt[v] = (uint64_t)(e - s);
        if (out_len) out_len[v] = len;
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// ---------------------------------------------------------------------------
// single 3-bit level, both strands (the twin of fmx_sfx_f3_p2_kernel on the front end of fmx_count_f3_p2rc_kernel;
// 4 <= max_character <= 7, so every code and every complemented code is a symbol of the index).
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_sfx_f3_p2rc_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, uint32_t mc, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2rc_split(gid, ngroups);
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t k = gid, base = 0, win = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, jw = 0, s = 0, e = 0, len = 0;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      const uint64_t pbeg = off[k], pend = off[k + 1];
      // offsets that go backwards or leave the pattern stream: refuse, do not read (j = 0 from here on)
      const bool badoff = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      j = (badoff || n < mc) ? 0u : (uint32_t)(pend - pbeg);   // (0, n) below min_count: no step can pass
      if (badoff && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      base = rc ? pend : pbeg;
      s = 0;
      e = badoff ? 0u : n;
      len = 0;
      jw = j;
      if (j) {
        const uint32_t cnt = j > 32u ? 32u : j;
        const uint64_t raw = fmx_p2rc_raw(words, rc, base, j, cnt);
        jw = j - cnt;
        win = fmx_p2rc_steps(raw, rc);
        if (KM && j >= kmer_k) {                         // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          if (kmer_bits == 2u) code = fmx_p2rc_code2(raw, rc, kmer_k);
          else (void)fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);   // codes 0..3: always symbols
          FMX_TOUCH_G0N(g, &kmer[code]);
          const uint2 se = kmer[code];
          if (se.y - se.x >= mc) {
            s = se.x; e = se.y;
            j -= kmer_k; len = kmer_k;
            win >>= 2u * kmer_k;
          }
        }
      }
      fresh = false;
    }
    bool done = (j == 0);
    if (!done) {
      const uint32_t c = ((uint32_t)win & 3u) + 1u;      // the symbol consumed next: <= 4 <= max_character
      const uint32_t rs = s >> 8, re = e >> 8;
      FMX_CHECK(rs < nrec && re < nrec);
      FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
      if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
      const uint4 a = rec[(size_t)rs * 8u + g];
      const uint4 b = rec[(size_t)re * 8u + g];
      // this step takes the window's last symbol and the pattern has more: the next window rides along
      const bool refill = j - jw == 1u && jw != 0u;
      const uint32_t cnt = jw > 32u ? 32u : jw;
      uint64_t raw = 0;
      if (refill) raw = fmx_p2rc_raw(words, rc, base, jw, cnt);
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
      if (ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        j--;
        win >>= 2u;
        if (refill) { win = fmx_p2rc_steps(raw, rc); jw -= cnt; }
        done = j == 0;
      }
    }
    if (done) {
      const uint64_t v = 2u * k + (rc ? 1u : 0u);        // slot 2 k: the pattern; 2 k + 1: its reverse complement
      if (g == 0) {
        if (out_s) out_s[v] = s;
        if (out_e) out_e[v] = e;
        if (out_cnt) out_cnt[v] = (uint64_t)(e - s);
        if (out_len) out_len[v] = len;
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
}

// the index of an EMPTY text, both strands: the start pair (0, 0) is below every min_count, so L = 0 and (0, 0) come
// back in both slots; the offsets are still checked and no word is read.  One lane per pattern.  (One strand is
// fmx_sfx_empty_kernel as it stands: it never reads a pattern.)
__global__ __launch_bounds__(FMX_BLOCK) void fmx_sfx_empty_p2rc_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    if (FMX_SPAN_BAD(off[k], off[k + 1], pmin, ptot)) atomicOr(status, 1u << FMX_ERR_ARG);
    for (uint64_t v = 2u * k; v < 2u * k + 2u; v++) {
      if (out_s) out_s[v] = 0;
      if (out_e) out_e[v] = 0;
      if (out_cnt) out_cnt[v] = 0;
      if (out_len) out_len[v] = 0;
    }
  }
}

// ---- launch: fmx_packed2_route()'s two rungs ----
int fmx_launch_sfx_packed2(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                           const uint64_t *d_s0e0, uint64_t min_count, uint64_t *d_s, uint64_t *d_e, uint64_t *d_cnt,
                           uint64_t *d_len, hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  if (r.shape == FMX_SHAPE_GROUP) {
    fmx_set_error(FMX_ERR_UNSUPPORTED, "packed patterns need a one-level FM index over u8 symbols on the 32-bit engine");
    return FMX_ERR_UNSUPPORTED;
  }
  if (npat == 0) return FMX_OK;
  if (idx->n == 0) {                                   // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_sfx_empty_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), dim3(FMX_BLOCK), 0, st,
                       dv.status, d_off, npat, d_s0e0, d_s, d_e, d_cnt, d_len);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  if (min_count == 0) min_count = 1;
  const uint32_t mc = min_count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)min_count;
  const dim3 grid(fmx_grid_for_groups(npat)), block(FMX_BLOCK);
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_pair_p2_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.pair_row0, dv.pair_row1, dv.status, dv.kmer, dv.kmer_k, d_words, d_off, npat, d_s0e0, mc,
                         d_s, d_e, d_cnt, d_len);
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_f3_p2_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character,
                         dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, d_words, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt,
                         d_len);
    });
  }
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

int fmx_launch_sfx_packed2_rc(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                              uint64_t min_count, uint64_t *d_s, uint64_t *d_e, uint64_t *d_cnt, uint64_t *d_len,
                              hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  if (r.shape == FMX_SHAPE_GROUP || dv.max_character < 4) {
    fmx_set_error(FMX_ERR_UNSUPPORTED, "both-strand packed patterns need a packed-pattern index with max_character >= 4");
    return FMX_ERR_UNSUPPORTED;
  }
  if (npat == 0) return FMX_OK;
  if (idx->n == 0) {                                   // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_sfx_empty_p2rc_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), dim3(FMX_BLOCK), 0, st,
                       dv.status, d_off, npat, d_s, d_e, d_cnt, d_len);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  if (min_count == 0) min_count = 1;
  const uint32_t mc = min_count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)min_count;
  const dim3 grid(fmx_grid_for_groups(2u * npat)), block(FMX_BLOCK);   // a group per strand of a pattern
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_pair_p2rc_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.pair_row0, dv.pair_row1, dv.status, dv.kmer, dv.kmer_k, d_words, d_off, npat, mc, d_s, d_e,
                         d_cnt, d_len);
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_f3_p2rc_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character,
                         dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, d_words, d_off, npat, mc, d_s, d_e, d_cnt, d_len);
    });
  }
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
