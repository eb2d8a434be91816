// fmx_packed_windows.h -- count EVERY length-k window of 2-bit packed DNA sequences, one strand or both
// (fmx_count_windows_packed2* / fmx_count_windows_packed2_rc*; included by fmx_query.hip after fmx_packed.h,
// fmx_packed_rc.h and fmx_packed_mstats.h, whose layout, fmx_p2_* / fmx_p2rc_* helpers and route it uses).
//
// A SLOT per sequence symbol, numbered by the window's start: slot t is the window [pmin + t, pmin + t + k) of the
// stream, pmin = seq_off[0].  Its result is what fmx_count_batch_packed2 gives for that window as a pattern of its own
// from (0, len); the both-strand call answers 2 total virtual slots u = 2 t + strand, strand 1 the window's reverse
// complement (R[x] = 5 - W[k - 1 - x]).  The steps, the collapsed-pair rule, the code-0 row correction and the early
// exit are those of fmx_count_pair_p2_kernel / fmx_count_f3_p2_kernel line for line.  What is new:
//   * the MARKER.  Whether slot t has a window depends on the sequence it lies in (t + k must not pass that sequence's
//     end), which is the one thing the slot number does not tell.  A pre-pass (fmx_p2w_mark_kernel) checks every
//     sequence's offsets once and leaves all-ones in out_count[u] of exactly the slots whose window fits, on cleared
//     arrays; an unmarked slot gives (0, 0, 0).  The hot kernels read no offset but seq_off[0] and seq_off[nseq].
//     Whatever a marker says, a kernel bounds its own reads: a window needs pmin + t + k <= ptot, and the only words
//     touched are words that hold a symbol of the window.
//   * the WORK SPLIT.  Groups stride over the windows, so the eight groups of a wave hold eight ADJACENT windows: their
//     word requests fall into the same one or two 8-byte words -- the stream costs 0.25 bytes per window where a batch
//     of patterns costs 8 bytes of words and 8 of offsets.  With both strands the strand is WAVE-UNIFORM, the split of
//     fmx_packed_rc.h: waves 2 p and 2 p + 1 of a block serve the same eight windows, one strand each.  (Strand per
//     group, the slot's parity, was measured first: a wave then steps as long as its longest strand, and where one
//     strand matches and the other ends early -- every read of a genome -- half its lanes idle)
//   * the PIPELINE.  A group requests the marker and both stream words of its NEXT slot under the steps of the current
//     one (request()); a window starts with its words in registers and goes straight to the k-mer table entry.
//   * the WINDOW is fmx_packed.h's / fmx_packed_rc.h's: strand 0 the backward funnel from E = start + k, reversed once
//     for the steps; strand 1 the forward funnel from start, complemented.  For k <= 32 no step loads a stream word;
//     for k > 32 the refill is the count twins': one wait per 32 symbols in the pair kernel, with a step's record loads
//     in the one-symbol kernel.
#pragma once

// out_count of every virtual slot cleared (a kernel, not a memset node: the call may be captured and replayed)
__global__ __launch_bounds__(FMX_BLOCK) void fmx_p2w_clear_kernel(uint64_t nslot, uint64_t *__restrict__ out_cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nslot; u += stride) out_cnt[u] = 0;
}

// the offsets of every sequence checked once (FMX_ERR_ARG as in the count kernels) and the slots marked whose window
// fits its sequence, never at or above the slot count.  A group per sequence; a long sequence is shared by 2^lsplit
// groups that take its slots in interleaved runs of eight (one sequence of 2^20 symbols is not one group's work).
template <bool RC>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_p2w_mark_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t nseq, uint64_t total, uint64_t k, uint32_t lsplit,
    uint64_t *__restrict__ out_cnt) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = off[nseq], pmin = off[0];
  if (gid == 0 && g == 0 && (ptot < pmin || ptot - pmin != total)) atomicOr(status, 1u << FMX_ERR_ARG);
  const uint64_t nslot = RC ? 2u * total : total;
  for (uint64_t q = gid; q < (nseq << lsplit); q += ngroups) {
    const uint64_t i = q >> lsplit, y = q & ((1ull << lsplit) - 1u);
    const uint64_t pbeg = off[i], pend = off[i + 1];
    if (FMX_SPAN_BAD32(pbeg, pend, pmin, ptot)) {
      if (g == 0 && y == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      continue;
    }
    const uint64_t m = pend - pbeg;
    if (m < k) continue;                                   // no window at all
    const uint64_t nmark = (RC ? 2u : 1u) * (m - k + 1u), u0 = (RC ? 2u : 1u) * (pbeg - pmin);
    for (uint64_t x = y * FMX_GROUP + g; x < nmark && u0 + x < nslot; x += (uint64_t)FMX_GROUP << lsplit)
      out_cnt[u0 + x] = ~0ull;
  }
}

// the group's first window and its stride over windows; -> the strand of its wave.  Both strands: fmx_p2rc_split(), the
// waves of a block alternate strands and waves 2 p, 2 p + 1 serve the same eight windows.  The slot of window t.
template <bool RC>
__device__ __forceinline__ bool fmx_p2w_split(uint64_t &gid, uint64_t &ngroups) {
  if (RC) return fmx_p2rc_split(gid, ngroups);
  gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  return false;
}
#define FMX_P2W_SLOT(t) (RC ? 2u * (t) + (rc ? 1u : 0u) : (t))

// ---------------------------------------------------------------------------
// every window with the pair index (the twin of fmx_count_pair_p2_kernel / fmx_count_pair_p2rc_kernel; max_character
// == 4, kmer_bits == 2, the dispatcher's rule).  `base` is the window's first symbol on strand 0 and the symbol after
// its last on strand 1: the unread edge is base + j there, base - j here.
// ---------------------------------------------------------------------------
template <bool KM, bool RC>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_win_pair_p2_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t nseq, uint64_t total, uint32_t k, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2w_split<RC>(gid, ngroups);

  uint64_t t = gid, base = 0, win = 0;
  bool active = t < total, fresh = true;
  uint32_t j = 0, s = 0, e = 0;
  uint32_t jw = 0;           // of the j unread symbols, those that are not in `win`
  uint32_t nsteps = 0;
  const uint64_t ptot = off[nseq], pmin = off[0];
  const uint64_t span = ptot >= pmin ? ptot - pmin : 0;
  const uint32_t cnt0 = k > 32u ? 32u : k;                 // symbols of a window's first fill
  // the group's NEXT slot travels under the current window's steps: its marker and the two words its first fill is cut
  // of (the same word twice when the fill does not straddle)
  uint64_t nm = 0, na = 0, nb = 0;
  auto request = [&](uint64_t tn) {
    if (tn >= total) return;
    nm = out_cnt[FMX_P2W_SLOT(tn)];
    if (tn + k <= span) {                                  // every symbol of the window is a symbol of the call
      const uint64_t B = pmin + tn, E = B + k;
      na = words[rc ? B >> 5 : (E - 1u) >> 5];
      nb = words[rc ? (B + cnt0 - 1u) >> 5 : (E - cnt0) >> 5];
    }
  };
  request(t);
  uint64_t wa = 0, wb = 0;
  while (active) {
    if (fresh) {
      const uint64_t m = nm;
      wa = na; wb = nb;
      request(t + ngroups);
      const bool fit = m == ~0ull && t + k <= span;
      base = pmin + t + (rc ? k : 0u);
      s = 0;
      e = fit ? n : 0u;
      j = fit ? k : 0u;
      jw = j;                                              // no window yet
    }
    // (re)fill the window: at the start of a window (its words are here already) and whenever fewer than two of its
    // symbols are left while it has more -- one wait per 32 symbols
    if (j - jw < 2u && jw != 0u) {
      const uint32_t cnt = j > 32u ? 32u : j;
      uint64_t raw;
      if (fresh) raw = rc ? fmx_p2_funnel_fwd(wa, wb, base - j) : fmx_p2_funnel(wa, wb, base + j);
      else raw = fmx_p2rc_raw(words, RC && rc, base, j, cnt);
      jw = j - cnt;
      win = fmx_p2rc_steps(raw, RC && rc);
      if (KM && fresh && j >= kmer_k) {                    // the first kmer_k steps from the table
        const uint32_t code = fmx_p2rc_code2(raw, RC && rc, kmer_k);
        FMX_TOUCH_G0N(g, &kmer[code]);
        const uint2 se = kmer[code];
        s = se.x;
        e = se.y;
        j = se.x == se.y ? 0u : j - kmer_k;                // empty already: the reference's break
        win >>= 2u * kmer_k;
        nsteps += kmer_k;
      }
    }
    fresh = false;
    bool done = (j == 0);
    if (!done) {
      const uint32_t code = (uint32_t)win & 15u;           // (c1 - 1) * 4 + (c2 - 1): c2 the symbol consumed first
      const uint32_t c2 = (code & 3u) + 1u;
      uint32_t used;
      if (j - jw >= 2u) {
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
        used = 2;
        if (ns == ne) {
          // would the reference already have stopped after the first symbol alone?
          FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
          FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
          if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
          const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
          const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
          const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));
          const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));
          if (s1 == e1) { ns = s1; ne = e1; used = 1; }
        }
        s = ns; e = ne;
      } else {
        FMX_CHECK((s >> 8) < n / 256u + 1u && (e >> 8) < n / 256u + 1u);
        FMX_TOUCH_G0(g, &rec1[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &rec1[(size_t)(e >> 8) * 8u]);
        const uint4 a1 = rec1[(size_t)(s >> 8) * 8u + g];
        const uint4 b1 = rec1[(size_t)(e >> 8) * 8u + g];
        const uint32_t s1 = fmx_group_sum(fmx_piece_rank<3>(a1, s & 255u, c2, g));  // wrapper.rs:109
        const uint32_t e1 = fmx_group_sum(fmx_piece_rank<3>(b1, e & 255u, c2, g));  // wrapper.rs:110
        s = s1; e = e1;
        used = 1;
      }
      nsteps += used;
      j -= used;
      win >>= 2u * used;
      if (s == e || j == 0) done = true;                   // wrapper.rs:111-113
    }
    if (done) {
      const uint64_t u = FMX_P2W_SLOT(t);
      if (g == 0) {
        if (out_s) out_s[u] = s;
        if (out_e) out_e[u] = e;
        out_cnt[u] = (uint64_t)(e - s);
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// ---------------------------------------------------------------------------
// every window on a single 3-bit level (the twin of fmx_count_f3_p2_kernel / fmx_count_f3_p2rc_kernel): one symbol per
// step out of the window; the fill that follows is requested in the step that consumes the last symbol of the current
// one, together with that step's two record loads.  max_character may be below 4 in the single-strand call: a code that
// is no symbol of the index is refused when it is reached.  RC: max_character >= 4, the dispatcher's rule.
// ---------------------------------------------------------------------------
template <bool KM, bool RC>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_win_f3_p2_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t nseq, uint64_t total, uint32_t k, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2w_split<RC>(gid, ngroups);
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t t = gid, base = 0, win = 0;
  bool active = t < total, fresh = true;
  uint32_t j = 0, jw = 0, s = 0, e = 0, nsteps = 0;
  const uint64_t ptot = off[nseq], pmin = off[0];
  const uint64_t span = ptot >= pmin ? ptot - pmin : 0;
  const uint32_t cnt0 = k > 32u ? 32u : k;                 // symbols of a window's first fill
  uint64_t nm = 0, na = 0, nb = 0;                         // the group's next slot: see fmx_win_pair_p2_kernel
  auto request = [&](uint64_t tn) {
    if (tn >= total) return;
    nm = out_cnt[FMX_P2W_SLOT(tn)];
    if (tn + k <= span) {                                  // every symbol of the window is a symbol of the call
      const uint64_t B = pmin + tn, E = B + k;
      na = words[rc ? B >> 5 : (E - 1u) >> 5];
      nb = words[rc ? (B + cnt0 - 1u) >> 5 : (E - cnt0) >> 5];
    }
  };
  request(t);
  while (active) {
    if (fresh) {
      const uint64_t m = nm, wa = na, wb = nb;
      request(t + ngroups);
      const bool fit = m == ~0ull && t + k <= span;
      base = pmin + t + (rc ? k : 0u);
      s = 0;                 // (0, len)   wrapper.rs:41
      e = fit ? n : 0u;
      j = fit ? k : 0u;
      jw = j;
      if (j) {
        const uint64_t raw = rc ? fmx_p2_funnel_fwd(wa, wb, base - j) : fmx_p2_funnel(wa, wb, base + j);
        jw = j - cnt0;
        win = fmx_p2rc_steps(raw, RC && rc);
        if (KM && j >= kmer_k) {                           // the first kmer_k steps from the table
          uint32_t code;
          bool ok = true;
          if (kmer_bits == 2u && max_character >= 4u) code = fmx_p2rc_code2(raw, RC && rc, kmer_k);
          else ok = fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);
          if (ok) {
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            s = se.x;
            e = se.y;
            j = se.x == se.y ? 0u : j - kmer_k;            // empty already: the reference's break
            win >>= 2u * kmer_k;
            nsteps += kmer_k;
          }
        }
      }
      fresh = false;
    }
    bool done = (j == 0);
    if (!done) {
      const uint32_t c = ((uint32_t)win & 3u) + 1u;        // the symbol consumed next
      if (c > max_character) {                             // reference: panic on cs[c]
        if (g == 0) atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE);
        s = 0; e = 0; done = true;
      } else {
        const uint32_t rs = s >> 8, re = e >> 8;
        FMX_CHECK(rs < nrec && re < nrec);
        FMX_TOUCH_G0(g, &rec[(size_t)rs * 8u]);
        if (re != rs) FMX_TOUCH_G0(g, &rec[(size_t)re * 8u]);
        const uint4 a = rec[(size_t)rs * 8u + g];
        const uint4 b = rec[(size_t)re * 8u + g];
        // this step takes the window's last symbol and the sequence window has more: the next fill rides along
        const bool refill = j - jw == 1u && jw != 0u;
        const uint32_t cnt = jw > 32u ? 32u : jw;
        uint64_t raw = 0;
        if (refill) raw = fmx_p2rc_raw(words, RC && rc, base, jw, cnt);
        const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));   // wrapper.rs:109
        const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));   // wrapper.rs:110
        s = ns; e = ne;
        j--;
        nsteps++;
        win >>= 2u;
        if (refill) { win = fmx_p2rc_steps(raw, RC && rc); jw -= cnt; }
        if (ns == ne || j == 0) done = true;               // wrapper.rs:111-113
      }
    }
    if (done) {
      const uint64_t u = FMX_P2W_SLOT(t);
      if (g == 0) {
        if (out_s) out_s[u] = s;
        if (out_e) out_e[u] = e;
        out_cnt[u] = (uint64_t)(e - s);                    // wrapper.rs:132-134
      }
      t += ngroups;
      active = t < total;
      fresh = true;
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// the index of an EMPTY text: every interval is (0, 0); the first step's symbol of a window that fits is still checked
// (strand 0: its last symbol; with both strands every code is a symbol of the index).  One lane per virtual slot.
template <bool RC>
__global__ __launch_bounds__(FMX_BLOCK) void fmx_p2w_empty_kernel(
    uint32_t max_character, uint32_t *status, const uint64_t *__restrict__ words, const uint64_t *__restrict__ off,
    uint64_t nseq, uint64_t nslot, uint32_t k, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *out_cnt) {
  const uint64_t ptot = off[nseq], pmin = off[0];
  const uint64_t span = ptot >= pmin ? ptot - pmin : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nslot; u += stride) {
    const uint64_t t = RC ? u >> 1 : u, last = pmin + t + k - 1u;
    if (!RC && out_cnt[u] == ~0ull && t + k <= span &&
        ((uint32_t)(words[last >> 5] >> (2u * ((uint32_t)last & 31u))) & 3u) + 1u > max_character)
      atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE);        // the first step's cs[c]
    if (out_s) out_s[u] = 0;
    if (out_e) out_e[u] = 0;
    out_cnt[u] = 0;
  }
}

// ---- launch: the clear and the marker pass, then fmx_packed2_route()'s two rungs or the empty text.  The caller has
// refused a handle the route does not serve (fmx_packed2_served / fmx_packed2_rc_served), a NULL d_cnt and a k outside
// [1, 2^32); nseq > 0.  `total` is the span of the offsets, the arrays have total entries, or 2 total with both. ----
int fmx_launch_count_windows_packed2(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off,
                                     uint64_t nseq, uint64_t total, uint64_t k, uint64_t *d_s, uint64_t *d_e,
                                     uint64_t *d_cnt, bool both, hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  const uint64_t nslot = both ? 2u * total : total;
  const dim3 block(FMX_BLOCK), lanes(fmx_grid_for_groups((nslot + 7) / 8));
  auto strands = [&](auto f) { if (both) f(std::true_type{}); else f(std::false_type{}); };
  if (nslot) hipLaunchKernelGGL(fmx_p2w_clear_kernel, lanes, block, 0, st, nslot, d_cnt);
  uint32_t lsplit = 0;                                     // a group marks about 512 slots: 64 stores per lane
  while (lsplit < 12u && (nseq << (lsplit + 9u)) < total) lsplit++;
  strands([&](auto rc) {
    hipLaunchKernelGGL(fmx_p2w_mark_kernel<decltype(rc)::value>, dim3(fmx_grid_for_groups(nseq << lsplit)), block, 0,
                       st, dv.status, d_off, nseq, total, k, lsplit, d_cnt);
  });
  FMX_HIP(hipGetLastError());
  if (nslot == 0) return FMX_OK;                     // (the marker pass has compared the offsets with it)
  if (idx->n == 0) {                                 // no record of any structure may be probed
    strands([&](auto rc) {
      hipLaunchKernelGGL(fmx_p2w_empty_kernel<decltype(rc)::value>, lanes, block, 0, st, dv.max_character, dv.status,
                         d_words, d_off, nseq, nslot, (uint32_t)k, d_s, d_e, d_cnt);
    });
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  fmx_time_begin(idx, st);
  uint64_t *steps = idx->timing == 1 ? idx->d_steps : nullptr;
  const dim3 grid(fmx_grid_for_groups(nslot));
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      strands([&](auto rc) {
        hipLaunchKernelGGL((fmx_win_pair_p2_kernel<decltype(km)::value, decltype(rc)::value>), grid, block, 0, st,
                           dv.bw.lv[0].rec, dv.pair_rec, dv.n, dv.pair_row0, dv.pair_row1, dv.kmer, dv.kmer_k, d_words,
                           d_off, nseq, total, (uint32_t)k, d_s, d_e, d_cnt, steps);
      });
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      strands([&](auto rc) {
        hipLaunchKernelGGL((fmx_win_f3_p2_kernel<decltype(km)::value, decltype(rc)::value>), grid, block, 0, st,
                           dv.bw.lv[0].rec, dv.n, dv.max_character, dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, d_words,
                           d_off, nseq, total, (uint32_t)k, d_s, d_e, d_cnt, steps);
      });
    });
  }
  fmx_time_end(idx, st);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
