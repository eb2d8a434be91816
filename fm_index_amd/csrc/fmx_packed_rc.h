// fmx_packed_rc.h -- count BOTH STRANDS of 2-bit packed DNA patterns in one launch (fmx_count_batch_packed2_rc*;
// included by fmx_query.hip after fmx_packed.h, whose layout, fmx_p2_* helpers and route it uses).
//
// The batch is 2 npat virtual patterns v = 2 k + strand: strand 0 is pattern k as written, strand 1 its reverse
// complement R, R[t] = 5 - P[m - 1 - t] (code x <-> x ^ 3).  Backward search of R consumes comp(P[0]), comp(P[1]), ...:
// it reads the pattern's own stream FRONT TO BACK with every code inverted, so R is never written down anywhere.
//
// Work split.  The strand is WAVE-UNIFORM: the waves of a block alternate strands, waves 2 p and 2 p + 1 serve the same
// eight patterns at the same time (the second reader of a word or an offset pair hits cache), and a group keeps its
// strand for its lifetime -- its stride over k is the number of group PAIRS of the grid.  The front-end choice is a
// scalar branch; the two strands of a pattern are never two chains of one group.
//
// Both strands keep the STEPS WINDOW of fmx_packed.h: `win & 3` is the symbol to consume next, `win & 15` the pair
// record's code (c1 - 1) * 4 + (c2 - 1), a step shifts right; `j` counts the unread symbols, `jw` those of them that
// are not in the window.  The front ends differ:
//   strand 0   fmx_packed.h's: symbols [E - cnt, E), E = pbeg + j, by the backward funnel (stream order), reversed for
//              the steps; the k-mer code is a shift of the stream-order window.
//   strand 1   symbols [B, B + cnt), B = pend - j, by a FORWARD funnel from word B / 32 and -- only when the window
//              straddles -- the word after it: the next symbol to consume is in the low two bits already, so there is
//              no reversal; the window is complemented once per fill (~).  Fields beyond cnt belong to neighbours and
//              are never consumed.  The k-mer code is the one thing that needs the reversal here: the top 2 kmer_k
//              bits of fmx_p2_reverse(window).  Tables of another code width recode from the window as it stands.
// Neither front end touches a word without a symbol of the pattern itself.  max_character >= 4 (the dispatcher refuses
// smaller alphabets), so every code and every complemented code is a symbol of the index: no symbol-range case.
#pragma once

static_assert(FMX_BLOCK % 128 == 0, "waves pair up inside a block");

// symbols [B, B + 32) of the stream, symbol B in the low two bits: lo = word B / 32, hi = the word after it (its value
// matters only where the window reaches beyond word B / 32)
__device__ __forceinline__ uint64_t fmx_p2_funnel_fwd(uint64_t lo, uint64_t hi, uint64_t B) {
  const uint32_t sh = 2u * ((uint32_t)B & 31u);
  return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}
__device__ __forceinline__ bool fmx_p2_straddles_fwd(uint64_t B, uint32_t cnt) { return ((B + cnt - 1u) >> 5) != (B >> 5); }
// the RAW window of the `cnt` symbols a strand consumes next when `left` of its symbols are unread (1 <= cnt <= 32,
// cnt <= left): strand 0 the stream-order window of [base + left - cnt, base + left), base = pbeg; strand 1 the
// forward window of [base - left, base - left + cnt), base = pend.  Both loads issued before the first use.
__device__ __forceinline__ uint64_t fmx_p2rc_raw(const uint64_t *__restrict__ words, bool rc, uint64_t base,
                                                 uint32_t left, uint32_t cnt) {
  if (!rc) return fmx_p2_load_window(words, base + left, cnt);
  const uint64_t B = base - left;
  const uint64_t lo = words[B >> 5];
  uint64_t hi = 0;
  if (fmx_p2_straddles_fwd(B, cnt)) hi = words[(B >> 5) + 1u];
  return fmx_p2_funnel_fwd(lo, hi, B);
}
// raw window -> steps window, and -> the 2-bit k-mer table code of its first kk symbols to consume
__device__ __forceinline__ uint64_t fmx_p2rc_steps(uint64_t raw, bool rc) { return rc ? ~raw : fmx_p2_reverse(raw); }
__device__ __forceinline__ uint32_t fmx_p2rc_code2(uint64_t raw, bool rc, uint32_t kk) {
  return (uint32_t)((rc ? fmx_p2_reverse(~raw) : raw) >> (64u - 2u * kk));
}
// strand of this wave, and the group's first pattern / the stride over patterns (group PAIRS of the grid)
__device__ __forceinline__ bool fmx_p2rc_split(uint64_t &gid, uint64_t &ngroups) {
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  gid = ((uint64_t)blockIdx.x * (FMX_BLOCK / 128) + (wv >> 1)) * 8u + ((threadIdx.x & 63u) >> 3);
  ngroups = (uint64_t)gridDim.x * (FMX_BLOCK / 128) * 8u;
  return (wv & 1u) != 0u;
}

// ---------------------------------------------------------------------------
// both strands with the pair index (the twin of fmx_count_pair_p2_kernel; max_character == 4, kmer_bits == 2).
// Steps, collapsed-pair rule, code-0 row correction and the odd remainder's single step are that kernel's, line for
// line; so is the two-deep pipeline -- the offsets of the pattern after next in flight, the next pattern's admitted
// offsets and its FIRST WORD in flight: word (pend - 1) / 32 on strand 0, word pbeg / 32 on strand 1.
// `base` is pbeg on strand 0 and pend on strand 1: the window's edge is base + j there, base - j here.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_count_pair_p2rc_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    uint32_t *status, const uint2 *__restrict__ kmer, uint32_t kmer_k, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2rc_split(gid, ngroups);

  uint64_t k = gid;
  bool active = k < npat, fresh = true;
  uint64_t base = 0, win = 0, w0 = 0;
  uint32_t j = 0, s = 0, e = 0;
  uint32_t jw = 0;           // of the j unread symbols, those that are not in `win`
  uint32_t nsteps = 0;
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
    nj = (nbad || !live) ? 0u : (uint32_t)(pend - pbeg);
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
      if (KM && fresh && j >= kmer_k) {                // the first kmer_k steps from the table
        const uint32_t code = fmx_p2rc_code2(raw, rc, kmer_k);
        FMX_TOUCH_G0N(g, &kmer[code]);
        const uint2 se = kmer[code];
        s = se.x;
        e = se.y;
        j = se.x == se.y ? 0u : j - kmer_k;            // empty already: the reference's break
        win >>= 2u * kmer_k;
        nsteps += kmer_k;
      }
    }
    fresh = false;
    bool done = (j == 0);
    if (!done) {
      const uint32_t code = (uint32_t)win & 15u;       // (c1 - 1) * 4 + (c2 - 1): c2 the symbol consumed first
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
      if (s == e || j == 0) done = true;               // wrapper.rs:111-113
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
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// ---------------------------------------------------------------------------
// both strands, single 3-bit level (the twin of fmx_count_f3_p2_kernel; 4 <= max_character <= 7): one symbol per step
// out of the window; the window that follows is requested in the step that consumes the last symbol of the current
// one, together with that step's two record loads.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_count_f3_p2rc_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  uint64_t gid, ngroups;
  const bool rc = fmx_p2rc_split(gid, ngroups);
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t k = gid, base = 0, win = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, jw = 0, s = 0, e = 0, nsteps = 0;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      const uint64_t pbeg = off[k], pend = off[k + 1];
      // offsets that go backwards or leave the pattern stream: refuse, do not read (j = 0 from here on)
      const bool badoff = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      j = badoff ? 0u : (uint32_t)(pend - pbeg);
      if (badoff && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      base = rc ? pend : pbeg;
      s = 0;                 // (0, len)   wrapper.rs:41
      e = badoff ? 0u : n;
      jw = j;
      if (j) {
        const uint32_t cnt = j > 32u ? 32u : j;
        const uint64_t raw = fmx_p2rc_raw(words, rc, base, j, cnt);
        jw = j - cnt;
        win = fmx_p2rc_steps(raw, rc);
        if (KM && j >= kmer_k) {                       // the first kmer_k steps from the table
          uint32_t code;
          if (kmer_bits == 2u) code = fmx_p2rc_code2(raw, rc, kmer_k);
          else (void)fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);   // codes 0..3: always symbols
          FMX_TOUCH_G0N(g, &kmer[code]);
          const uint2 se = kmer[code];
          s = se.x;
          e = se.y;
          j = se.x == se.y ? 0u : j - kmer_k;          // empty already: the reference's break
          win >>= 2u * kmer_k;
          nsteps += kmer_k;
        }
      }
      fresh = false;
    }
    bool done = (j == 0);
    if (!done) {
      const uint32_t c = ((uint32_t)win & 3u) + 1u;    // the symbol consumed next: <= 4 <= max_character
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
      const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));   // wrapper.rs:109
      const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));   // wrapper.rs:110
      s = ns; e = ne;
      j--;
      nsteps++;
      win >>= 2u;
      if (refill) { win = fmx_p2rc_steps(raw, rc); jw -= cnt; }
      if (ns == ne || j == 0) done = true;             // wrapper.rs:111-113
    }
    if (done) {
      const uint64_t v = 2u * k + (rc ? 1u : 0u);      // slot 2 k: the pattern; 2 k + 1: its reverse complement
      if (g == 0) {
        if (out_s) out_s[v] = s;
        if (out_e) out_e[v] = e;
        if (out_cnt) out_cnt[v] = (uint64_t)(e - s);   // wrapper.rs:132-134
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// the index of an EMPTY text: every interval of both strands is (0, 0); the offsets are still checked, no word is read
// (every code is a symbol of the index).  One lane per pattern, both of its slots.
__global__ __launch_bounds__(FMX_BLOCK) void fmx_count_empty_p2rc_kernel(
    uint32_t *status, const uint64_t *__restrict__ off, uint64_t npat, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    if (FMX_SPAN_BAD(off[k], off[k + 1], pmin, ptot)) atomicOr(status, 1u << FMX_ERR_ARG);
    for (uint64_t v = 2u * k; v < 2u * k + 2u; v++) {
      if (out_s) out_s[v] = 0;
      if (out_e) out_e[v] = 0;
      if (out_cnt) out_cnt[v] = 0;
    }
  }
}

// ---- launch: fmx_packed2_route()'s two rungs, for alphabets in which every complemented code is a symbol ----
bool fmx_packed2_rc_served(const fmx_index *idx) {
  return fmx_packed2_route(idx, idx->dev).shape != FMX_SHAPE_GROUP && idx->dev.max_character >= 4;
}

int fmx_launch_count_packed2_rc(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                                uint64_t *d_s, uint64_t *d_e, uint64_t *d_cnt, hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  if (r.shape == FMX_SHAPE_GROUP || dv.max_character < 4) {
    fmx_set_error(FMX_ERR_UNSUPPORTED, "both-strand packed patterns need a packed-pattern index with max_character >= 4");
    return FMX_ERR_UNSUPPORTED;
  }
  if (npat == 0) return FMX_OK;
  if (idx->n == 0) {                                   // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_count_empty_p2rc_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), dim3(FMX_BLOCK), 0, st,
                       dv.status, d_off, npat, d_s, d_e, d_cnt);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  fmx_time_begin(idx, st);
  uint64_t *steps = idx->timing == 1 ? idx->d_steps : nullptr;
  const dim3 grid(fmx_grid_for_groups(2u * npat)), block(FMX_BLOCK);   // a group per strand of a pattern
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_count_pair_p2rc_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.pair_row0, dv.pair_row1, dv.status, dv.kmer, dv.kmer_k, d_words, d_off, npat, d_s, d_e,
                         d_cnt, steps);
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_count_f3_p2rc_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character,
                         dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, d_words, d_off, npat, d_s, d_e, d_cnt, steps);
    });
  }
  fmx_time_end(idx, st);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
