// fmx_suffix.h -- batched longest-suffix match on the 32-bit engine (fmx_suffix_match_batch*; included by fmx_query.hip).
//
// An ADDITION with no counterpart in the crate: the closest is Search::search (wrapper.rs:99-124) repeated one symbol
// at a time until count() drops below min_count.  For every pattern:
//     (s, e) = start pair; L = 0
//     for c in pattern reversed:
//         if c > max_character: break                      # ends the match, NOT an error
//         s' = lf_map2(c, s); e' = lf_map2(c, e)
//         if e' - s' < min_count: break
//         s = s'; e = e'; L += 1
// Interval sizes never grow along the loop, so whatever shortcut lands on an interval of >= min_count rows after t
// symbols has passed t intervals of >= min_count rows: a k-mer table entry that wide is the state after k steps, a
// pair probe that wide the state after two more.  An entry or probe below min_count says nothing about WHERE the match
// stopped and the steps are taken one at a time.
//
// One kernel per count kernel of fmx_query.hip and rung of its dispatch ladder (fmx_route), same shapes (8-lane groups,
// one dwordx4 per lane and record, DPP sums, the next symbol with the record loads, endpoint per lane for RLFM).
// `mc` is min_count clamped to 1 .. 2^32 - 1 by the launcher (n < 2^32 - 16: a larger value matches nothing either).
#pragma once

// group per pattern, every kind and level count (the twin of fmx_count_kernel)
template <int KIND, int NL, bool KM, int SM>
__global__ __launch_bounds__(FMX_BLOCK, 8) void fmx_sfx_kernel(
    FmxDev ix, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint32_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t k = gid;          // current pattern
  bool active = k < npat;
  bool fresh = true;         // pattern state not loaded yet
  uint64_t pbeg = 0;         // first symbol of the pattern
  uint32_t j = 0;            // symbols still to consume (from the back)
  uint32_t s = 0, e = 0, len = 0;
  uint32_t c = 0;            // symbol of the coming step (loaded one step ahead)

  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      j = (uint32_t)(pend - pbeg);
      // offsets that go backwards or leave the pattern buffer: refuse, do not read (j = 0 from here on)
      bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      s = 0; e = ix.n; len = 0;
      if (s0e0) {
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        bad |= s64 > ix.n || e64 > ix.n;                 // not a range of this index
      }
      if (bad) {
        if (g == 0) atomicOr(ix.status, 1u << FMX_ERR_ARG);
        s = 0; e = 0; j = 0;
      } else if (e < s || e - s < mc) {                  // a start pair below min_count: no step can pass
        j = 0;
      } else if (KM && !s0e0 && j >= ix.kmer_k) {        // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code((const uint8_t *)pat, pbeg + j, ix.kmer_k, ix.kmer_bits, ix.max_character, g, code)) {
          FMX_TOUCH_G0N(g, &ix.kmer[code]);
          const uint2 se = ix.kmer[code];
          if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= ix.kmer_k; len = ix.kmer_k; }
        }
      }
      c = j ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 1) : 0u;
      fresh = false;
    }
    bool done = j == 0 || c > ix.max_character;          // an absent symbol ends the match
    if (!done) {
      // the next symbol rides along with this step's record loads
      const uint32_t cn = j > 1 ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 2) : 0u;
      uint32_t ns = s, ne = e;
      fmx_lf_map2_pair<KIND, NL, SM>(ix, c, ns, ne, g);
      // (ne < ns: lf_map2(0, .) of a multi-pieces index is not monotone, multi_pieces.rs:147-153 -- below every min_count)
      if (ne < ns || ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        c = cn;
        j--;
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

// the index of an EMPTY text: the start pair (0, 0) is below every min_count, so L = 0 and the start pair come back;
// one lane per pattern, offsets and given ranges checked like everywhere else (the twin of fmx_count_empty_kernel)
__global__ __launch_bounds__(FMX_BLOCK) void fmx_sfx_empty_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0,
    uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt,
    uint64_t *__restrict__ out_len) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    const uint64_t a = off[k], b = off[k + 1];
    if (FMX_SPAN_BAD(a, b, pmin, ptot) || (s0e0 && (s0e0[2 * k] | s0e0[2 * k + 1]) != 0))
      atomicOr(status, 1u << FMX_ERR_ARG);
    if (out_s) out_s[k] = 0;
    if (out_e) out_e[k] = 0;
    if (out_cnt) out_cnt[k] = 0;
    if (out_len) out_len[k] = 0;
  }
}

// single 3-bit level (DNA): one 128-byte line per interval end and step (the twin of fmx_count_f3_kernel<1, false>)
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_sfx_f3_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint32_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t k = gid, pbeg = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, s = 0, e = 0, c = 0, len = 0;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      j = (uint32_t)(pend - pbeg);
      // offsets that go backwards or leave the pattern buffer: refuse, do not read (j = 0 from here on)
      bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
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
      } else if (KM && !s0e0 && j >= kmer_k) {           // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code(pat, pbeg + j, kmer_k, kmer_bits, max_character, g, code)) {
          FMX_TOUCH_G0N(g, &kmer[code]);
          const uint2 se = kmer[code];
          if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; }
        }
      }
      c = j ? pat[pbeg + j - 1] : 0u;                    // last symbol first
      fresh = false;
    }
    bool done = j == 0 || c > max_character;             // an absent symbol ends the match
    if (!done) {
      const uint32_t rs = s >> 8, re = e >> 8;
      FMX_CHECK(rs < nrec && re < nrec);
      FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
      if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
      const uint4 a = rec[(size_t)rs * 8u + g];
      const uint4 b = rec[(size_t)re * 8u + g];
      const uint32_t cn = j > 1 ? pat[pbeg + j - 2] : 0u;    // rides along with the record loads
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));
      if (ne - ns < mc) {
        done = true;                                     // keep the previous (s, e, len)
      } else {
        s = ns; e = ne; len++;
        c = cn;
        j--;
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

// the opt-in pair index (the twin of fmx_count_pair_kernel): while two symbols remain, both in 1..4, one probe of the
// 2-gram records per interval end advances two symbols when its result keeps >= min_count rows.  Otherwise the single
// step for the last symbol on the 1-gram records (the probe the count kernel makes when its pair step collapses):
// >= min_count rows -> taken, and the match ends there, the second symbol being known to fail; else nothing is taken.
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_sfx_pair_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n,
    uint32_t max_character, uint32_t row0, uint32_t row1, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits,
    const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint32_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t k = gid, pbeg = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, s = 0, e = 0, len = 0;
  uint32_t c2 = 0, c1 = 0;   // c2 = last unread symbol, c1 = the one before it
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  // the offsets of the group's NEXT pattern travel under the current pattern's steps
  uint64_t nbeg = active ? off[k] : 0, nend = active ? off[k + 1] : 0;
  while (active) {
    if (fresh) {
      pbeg = nbeg;
      const uint64_t pend = nend;
      if (k + ngroups < npat) { nbeg = off[k + ngroups]; nend = off[k + ngroups + 1]; }
      j = (uint32_t)(pend - pbeg);
      // offsets that go backwards or leave the pattern buffer: refuse, do not read (j = 0 from here on)
      bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
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
      } else if (KM && !s0e0 && j >= kmer_k) {           // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code(pat, pbeg + j, kmer_k, kmer_bits, max_character, g, code)) {
          FMX_TOUCH_G0N(g, &kmer[code]);
          const uint2 se = kmer[code];
          if (se.y - se.x >= mc) { s = se.x; e = se.y; j -= kmer_k; len = kmer_k; }
        }
      }
      c2 = j ? pat[pbeg + j - 1] : 0u;
      c1 = j > 1 ? pat[pbeg + j - 2] : 0u;
      fresh = false;
    }
    bool done = j == 0 || c2 > max_character;            // an absent symbol ends the match
    if (!done) {
      const bool pair = j >= 2 && (c2 - 1u) < 4u && (c1 - 1u) < 4u && c1 <= max_character;
      // the two symbols after these ride along with the record loads
      const uint32_t n1 = j > 2 ? pat[pbeg + j - 3] : 0u;
      const uint32_t n2 = j > 3 ? pat[pbeg + j - 4] : 0u;
      uint32_t used = 0;
      if (pair) {
        const uint32_t code = (c1 - 1u) * 4u + (c2 - 1u);
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
        done = pair || used == 0;                        // after a failed pair probe the second symbol is known to fail
      }
      len += used;
      j -= used;
      if (used == 2) { c2 = n1; c1 = n2; } else { c2 = c1; c1 = n1; }
      done |= j == 0;
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

// endpoint per lane (the twin of fmx_count_ep_kernel): lane 2q keeps s and lane 2q+1 keeps e of the group's q-th
// pattern, each with its own previous endpoint; the width of the stepped interval is formed from the pair's two lanes
// the way the count kernel forms `s == e`, and both lanes take the same decision.
template <int KIND, int NL, int SM, bool KM>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_sfx_ep_kernel(
    FmxDev ix, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint32_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  const uint32_t lane = threadIdx.x & 63u, g = lane & 7u, base = lane & ~7u;
  const uint32_t is_e = g & 1u;
  // pattern slots are dealt to the GROUPS first (slot = pair * ngroups + group), as in the count kernel
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) >> 3;
  const uint64_t slot = (uint64_t)(g >> 1) * ngroups + (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3);
  const uint64_t nslots = ngroups * 4u;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)

  uint64_t k = slot, pbeg = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, pos = 0, c = 0, len = 0;
  while (__any(active)) {
    if (active && fresh) {                               // (both lanes of a pair are here together)
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      j = (uint32_t)(pend - pbeg);
      bool bad = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      len = 0;
      uint32_t oth;                                      // the pair's other end
      if (s0e0) {
        const uint64_t mine = s0e0[2 * k + is_e], other = s0e0[2 * k + (is_e ^ 1u)];
        pos = (uint32_t)mine;
        oth = (uint32_t)other;
        bad |= mine > ix.n || other > ix.n;              // not a range of this index
      } else {
        pos = is_e ? ix.n : 0u;
        oth = is_e ? 0u : ix.n;
      }
      const uint32_t ss = is_e ? oth : pos, ee = is_e ? pos : oth;
      if (bad) {             // refuse, do not read
        if (is_e) atomicOr(ix.status, 1u << FMX_ERR_ARG);
        pos = 0; j = 0;
      } else if (ee < ss || ee - ss < mc) {              // a start pair below min_count: no step can pass
        j = 0;
      } else if (KM && !s0e0 && j >= ix.kmer_k) {        // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code_lane((const uint8_t *)pat, pbeg + j, ix.kmer_k, ix.kmer_bits, ix.max_character, code)) {
          FMX_TOUCH(&ix.kmer[code]);
          const uint2 se = ix.kmer[code];
          if (se.y - se.x >= mc) { pos = is_e ? se.y : se.x; j -= ix.kmer_k; len = ix.kmer_k; }
        }
      }
      c = j ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 1) : 0u;
      fresh = false;
    }
    if (active && j != 0 && c > ix.max_character) j = 0; // an absent symbol ends the match
    const bool stepping = active && j != 0;
    // the next symbol rides along with this step's probes
    const uint32_t cn = (stepping && j > 1) ? fmx_load_sym(pat, ix.sym_bytes, pbeg + j - 2) : 0u;
    const uint32_t np = KIND == FMX_KIND_RLFM
                            ? fmx_rlfm_ep_lf_map2<NL, (SM > 0 ? SM : 1)>(ix, stepping ? c : 0u, stepping ? pos : 0u, stepping, base, g)
                            : fmx_fm_ep_lf_map2<NL>(ix, stepping ? c : 0u, stepping ? pos : 0u, stepping, base, g);
    const uint32_t onp = fmx_dpp_xor1(np);               // the stepped other end
    if (stepping) {
      const uint32_t ns = is_e ? onp : np, ne = is_e ? np : onp;
      if (ne < ns || ne - ns < mc) {
        j = 0;                                           // keep the previous endpoint and len
      } else {
        pos = np;
        len++;
        c = cn;
        j--;
      }
    }
    const uint32_t other = fmx_dpp_xor1(pos);            // the pattern's other interval end
    if (active && j == 0) {
      if (is_e) {
        if (out_e) out_e[k] = pos;
        if (out_cnt) out_cnt[k] = pos >= other ? (uint64_t)(pos - other) : 0ull;   // (a given start pair with e < s holds no row)
        if (out_len) out_len[k] = len;
      } else if (out_s) {
        out_s[k] = pos;
      }
      k += nslots;
      active = k < npat;
      fresh = true;
    }
  }
}

// ---- launch: the ladder of fmx_route() (fmx_query.hip), every shape ----
int fmx_launch_suffix_match(const fmx_index *idx, const void *d_pat, const uint64_t *d_off, uint64_t npat,
                            const uint64_t *d_s0e0, uint64_t min_count, uint64_t *d_s, uint64_t *d_e,
                            uint64_t *d_cnt, uint64_t *d_len, hipStream_t st) {
  if (min_count == 0) min_count = 1;
  if (idx->is_wide) return fmxw_launch_suffix_match(idx, d_pat, d_off, npat, d_s0e0, min_count, d_s, d_e, d_cnt, d_len, st);
  const FmxDev dv = fmx_launch_dev(idx);
  if (npat == 0) return FMX_OK;
  if (idx->n == 0) {                                 // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_sfx_empty_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), dim3(FMX_BLOCK), 0, st,
                       dv.status, d_off, npat, d_s0e0, d_s, d_e, d_cnt, d_len);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  const FmxTune tn = fmx_tune();
  const FmxRoute r = fmx_route(idx, dv, tn, FMX_SHAPE_PAIR | FMX_SHAPE_F3 | FMX_SHAPE_EP | FMX_SHAPE_GROUP | FMX_HAS_KMER);
  const uint32_t mc = min_count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)min_count;
  const dim3 grid(fmx_grid_for_groups(npat)), block(FMX_BLOCK);
  const uint8_t *pat8 = (const uint8_t *)d_pat;
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_pair_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.max_character, dv.pair_row0, dv.pair_row1, dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, pat8,
                         d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len);
    });
  } else if (r.shape == FMX_SHAPE_F3) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_sfx_f3_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character, dv.status,
                         dv.kmer, dv.kmer_k, dv.kmer_bits, pat8, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len);
    });
  } else if (r.shape == FMX_SHAPE_EP) {
    const dim3 eb((unsigned)fmx_ep_count_blocks(npat, tn.ep_blocks));
    fmx_route_ep(r, [&](auto kind, auto nl, auto sm, auto km) {
      hipLaunchKernelGGL((fmx_sfx_ep_kernel<kind(), nl(), sm(), km()>), eb, block, 0, st, dv, d_pat, d_off, npat, d_s0e0,
                         mc, d_s, d_e, d_cnt, d_len);
    });
  } else {
    fmx_route_group(r, [&](auto kind, auto nl, auto sm, auto km) {
      hipLaunchKernelGGL((fmx_sfx_kernel<kind(), nl(), km(), sm()>), grid, block, 0, st, dv, d_pat, d_off, npat, d_s0e0,
                         mc, d_s, d_e, d_cnt, d_len);
    });
  }
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
