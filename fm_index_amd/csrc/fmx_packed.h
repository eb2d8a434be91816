// fmx_packed.h -- count on 2-bit packed DNA patterns (fmx_count_batch_packed2*; included by fmx_query.hip).
//
// The layout (include/fmx.h): symbol i of the pattern stream is the 2-bit value `symbol - 1` in bits
// [2 (i mod 32), 2 (i mod 32) + 2) of little-endian 64-bit word i / 32; i is numbered like pat_off.  A pattern may start
// and end anywhere inside a word.  Only symbols 1..4 can be written down, so the byte kernels' symbol-0 case and their
// validity reduction have no counterpart here; a code above max_character - 1 (max_character < 4) is refused when the
// search REACHES it, as the byte kernels refuse the symbol.
//
// Two kernels, the twins of fmx_count_pair_kernel and fmx_count_f3_kernel<1, false> (fmx_query.hip): the same 8-lane
// groups, one record line per lane, the same state machine (a group that finishes early picks up its next pattern
// while its wave-mates keep stepping), the same steps and the same early-exit rules -- with a pattern front end of
// their own:
//   * the WINDOW.  The unread end of a pattern, up to 32 symbols, is one 64-bit value.  It is cut out of the stream
//     with at most two 8-byte loads (every lane of the group asks for the same address: one request each) and a funnel
//     shift; the second load is issued only when the window straddles a word.  Only words that hold symbols of the
//     pattern itself are read, so nothing outside words pat_off[0] / 32 .. (pat_off[npat] - 1) / 32 is touched.  The
//     funnel leaves the window in STREAM order, the pattern's last unread symbol in the top two bits; stream bits that
//     belong to a neighbouring pattern (or to nobody) land in fields beyond the window's symbol count and are never
//     consumed.
//   * the K-MER CODE is the top 2 kmer_k bits of the stream-order window: stream order is the table's order (the symbol
//     consumed first in the top bits), so the byte kernels' gather or bit reversal is a shift here.  Tables of another
//     code width, and alphabets of fewer than four symbols (where a code may be out of range), recode in registers.
//   * the STEPS take their symbols from the REVERSED window (one 64-bit reversal of the 2-bit fields per 32 symbols):
//     `win & 15` is the pair record's code (c1 - 1) * 4 + (c2 - 1), `win & 3` the last unread symbol, and a step
//     shifts the window right.  No step issues a pattern load; a refill is one wait per 32 symbols in the pair kernel
//     and rides along with a step's record loads in the one-symbol kernel.
#pragma once

// the 2-bit fields of v in reverse order (bit reversal, then the two bits of every field swapped back)
__device__ __forceinline__ uint64_t fmx_p2_reverse(uint64_t v) {
  const uint64_t r = __brevll(v);
  return ((r & 0x5555555555555555ull) << 1) | ((r >> 1) & 0x5555555555555555ull);
}
// symbols [E - 32, E) of the stream in stream order, symbol E - 1 in the top two bits: hi = word (E - 1) / 32, lo = the
// word before it (its value matters only where the window reaches below word (E - 1) / 32)
__device__ __forceinline__ uint64_t fmx_p2_funnel(uint64_t hi, uint64_t lo, uint64_t E) {
  const uint32_t sh = 2u * ((uint32_t)E & 31u);
  return sh ? (hi << (64u - sh)) | (lo >> sh) : hi;
}
// word of the stream that holds the LAST of the symbols [E - cnt, E), and the word that holds the first when that is
// another one (1 <= cnt <= 32: the word before)
__device__ __forceinline__ uint64_t fmx_p2_word_hi(uint64_t E) { return (E - 1u) >> 5; }
__device__ __forceinline__ bool fmx_p2_straddles(uint64_t E, uint32_t cnt) { return ((E - cnt) >> 5) != ((E - 1u) >> 5); }
// the stream-order window of symbols [E - cnt, E): both loads issued before the first use
__device__ __forceinline__ uint64_t fmx_p2_load_window(const uint64_t *__restrict__ words, uint64_t E, uint32_t cnt) {
  const uint64_t hi = words[fmx_p2_word_hi(E)];
  uint64_t lo = 0;
  if (fmx_p2_straddles(E, cnt)) lo = words[(E - cnt) >> 5];
  return fmx_p2_funnel(hi, lo, E);
}
// fmx_kmer_code (fmx_device.h) of the first kk (<= 16, <= symbols in the window) symbols of a REVERSED window, for
// any code width; false when one of them is above max_character (then the stepwise path decides)
__device__ __forceinline__ bool fmx_p2_kmer_code(uint64_t win, uint32_t kk, uint32_t bits, uint32_t max_character,
                                                 uint32_t &code) {
  uint32_t bad = 0;
  code = 0;
  for (uint32_t t = 0; t < kk; t++) {                     // t-th symbol from the back
    const uint32_t cc = (uint32_t)(win >> (2u * t)) & 3u;
    bad |= (uint32_t)(cc >= max_character);
    code |= (cc & ((1u << bits) - 1u)) << (bits * (kk - 1u - t));
  }
  return bad == 0u;
}

// ---------------------------------------------------------------------------
// count with the pair index on a packed stream (the twin of fmx_count_pair_kernel; max_character == 4, so every code
// is a symbol of the index and kmer_bits == 2 -- the dispatcher sends smaller alphabets to the kernel below).
// Steps, collapsed-pair rule, code-0 row correction and the odd remainder's single step are the byte kernel's, line
// for line.  The pattern start is shorter by one wait: a group keeps a two-deep pipeline under its steps --
//     the offsets of the pattern AFTER NEXT (noff, in flight),
//     the admitted offsets of the NEXT pattern and its first stream word (nbeg, nj, nbad, nhi; the word in flight)
// -- so that a pattern starts with its window's word already in a register and goes straight to the table entry.
// (A refinement call does not prefetch the word: a pattern whose start pair is refused is never read.)
// SGPRs: see the note above fmx_count_pair_kernel -- 8 waves per SIMD must start.
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_count_pair_p2_kernel(
    const uint4 *__restrict__ rec1, const uint4 *__restrict__ rec2, uint32_t n, uint32_t row0, uint32_t row1,
    uint32_t *status, const uint2 *__restrict__ kmer, uint32_t kmer_k, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;

  uint64_t k = gid;
  bool active = k < npat, fresh = true;
  uint64_t pbeg = 0, win = 0, hi = 0;
  uint32_t j = 0, s = 0, e = 0;
  uint32_t jw = 0;           // `win` holds the unread symbols [jw, j) of the pattern, the last one in its low bits
  uint32_t nsteps = 0;
  bool badoff = false;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  typedef uint64_t fmx_u64x2 __attribute__((ext_vector_type(2), aligned(8)));
  fmx_u64x2 noff = {0, 0};
  uint64_t nbeg = 0, nhi = 0;
  uint32_t nj = 0;
  bool nbad = false;
  // noff (arrived; `live`: it belongs to a pattern) becomes the next pattern: its offsets are checked before anything
  // of it is read, its first word and the offsets of pattern `kn` are requested
  auto admit = [&](bool live, uint64_t kn) {
    nbeg = noff.x;
    const uint64_t pend = noff.y;
    nbad = live && FMX_SPAN_BAD32(nbeg, pend, pmin, ptot);
    nj = (nbad || !live) ? 0u : (uint32_t)(pend - nbeg);
    if (nj && !s0e0) nhi = words[fmx_p2_word_hi(pend)];
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
      if (s0e0) {
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        if (s64 > n || e64 > n || badoff) {            // not a range of this index: refuse, do not read
          if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
          s = 0; e = 0; j = 0;
        }
        if (j) hi = words[fmx_p2_word_hi(pbeg + j)];
      } else {
        s = 0;
        e = badoff ? 0u : n;
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
      if (KM && fresh && !s0e0 && j >= kmer_k) {       // the first kmer_k steps from the table
        const uint32_t code = (uint32_t)(str >> (64u - 2u * kmer_k));
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
      const uint32_t code = (uint32_t)win & 15u;       // (c1 - 1) * 4 + (c2 - 1): c2 the last unread symbol
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
          // would the reference already have stopped after the last symbol alone?
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
      const uint64_t kd = k;
      advance();
      admit(k + 2u * ngroups < npat, k + 3u * ngroups);
      if (g == 0) {
        if (out_s) out_s[kd] = s;
        if (out_e) out_e[kd] = e;
        if (out_cnt) out_cnt[kd] = (uint64_t)(e - s);
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
// count, single 3-bit level, on a packed stream (the twin of fmx_count_f3_kernel<1, false>): one symbol per step, taken
// from the window.  The window that follows is requested in the step that consumes the last symbol of the current one,
// together with that step's two record loads -- one wait serves all of them, and no step waits for the pattern.
// max_character may be below 4 here: a code that is no symbol of the index is refused when it is reached.
// (SGPRs capped like the pair kernels': uncapped, the table instantiation takes 90 and starts 7 waves per SIMD.)
// ---------------------------------------------------------------------------
template <bool KM>
__global__ __launch_bounds__(FMX_BLOCK) __attribute__((amdgpu_num_sgpr(80))) void fmx_count_f3_p2_kernel(
    const uint4 *__restrict__ rec, uint32_t n, uint32_t max_character, uint32_t *status,
    const uint2 *__restrict__ kmer, uint32_t kmer_k, uint32_t kmer_bits, const uint64_t *__restrict__ words,
    const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ s0e0, uint64_t *__restrict__ out_s,
    uint64_t *__restrict__ out_e, uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ steps_out) {
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  [[maybe_unused]] const uint32_t nrec = n / 256u + 1u;

  uint64_t k = gid, pbeg = 0, win = 0;
  bool active = k < npat, fresh = true;
  uint32_t j = 0, jw = 0, s = 0, e = 0, nsteps = 0;
  const uint64_t ptot = npat ? off[npat] : 0;   // symbols the caller declares behind `words`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  while (active) {
    if (fresh) {
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      // offsets that go backwards or leave the pattern stream: refuse, do not read (j = 0 from here on)
      const bool badoff = FMX_SPAN_BAD32(pbeg, pend, pmin, ptot);
      j = badoff ? 0u : (uint32_t)(pend - pbeg);
      if (badoff && g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
      if (s0e0) {            // Search::search on an existing Search (wrapper.rs:105-106)
        const uint64_t s64 = s0e0[2 * k], e64 = s0e0[2 * k + 1];
        s = (uint32_t)s64;
        e = (uint32_t)e64;
        if (s64 > n || e64 > n || badoff) {            // not a range of this index: refuse, do not read
          if (g == 0) atomicOr(status, 1u << FMX_ERR_ARG);
          s = 0; e = 0; j = 0;
        }
      } else {               // (0, len)   wrapper.rs:41
        s = 0;
        e = badoff ? 0u : n;
      }
      jw = j;
      if (j) {
        const uint32_t cnt = j > 32u ? 32u : j;
        const uint64_t str = fmx_p2_load_window(words, pbeg + j, cnt);
        jw = j - cnt;
        win = fmx_p2_reverse(str);
        if (KM && !s0e0 && j >= kmer_k) {              // the first kmer_k steps from the table
          uint32_t code;
          bool ok = true;
          if (kmer_bits == 2u && max_character >= 4u) code = (uint32_t)(str >> (64u - 2u * kmer_k));
          else ok = fmx_p2_kmer_code(win, kmer_k, kmer_bits, max_character, code);
          if (ok) {
            FMX_TOUCH_G0N(g, &kmer[code]);
            const uint2 se = kmer[code];
            s = se.x;
            e = se.y;
            j = se.x == se.y ? 0u : j - kmer_k;        // empty already: the reference's break
            win >>= 2u * kmer_k;
            nsteps += kmer_k;
          }
        }
      }
      fresh = false;
    }
    bool done = (j == 0);
    if (!done) {
      const uint32_t c = ((uint32_t)win & 3u) + 1u;    // last unread symbol: pattern.iter().rev()
      if (c > max_character) {                         // reference: panic on cs[c]
        if (g == 0) atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE);
        s = 0; e = 0; done = true;
      } else {
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
        const uint32_t ns = fmx_group_sum(fmx_piece_rank<3>(a, s & 255u, c, g));   // wrapper.rs:109
        const uint32_t ne = fmx_group_sum(fmx_piece_rank<3>(b, e & 255u, c, g));   // wrapper.rs:110
        s = ns; e = ne;
        j--;
        nsteps++;
        win >>= 2u;
        if (refill) { win = fmx_p2_reverse(str); jw -= cnt; }
        if (ns == ne || j == 0) done = true;           // wrapper.rs:111-113
      }
    }
    if (done) {
      if (g == 0) {
        if (out_s) out_s[k] = s;
        if (out_e) out_e[k] = e;
        if (out_cnt) out_cnt[k] = (uint64_t)(e - s);   // wrapper.rs:132-134
      }
      k += ngroups;
      active = k < npat;
      fresh = true;
    }
  }
  if (steps_out && g == 0 && nsteps)
    atomicAdd((unsigned long long *)steps_out, (unsigned long long)nsteps);
}

// the index of an EMPTY text (fmx_count_empty_kernel on a packed stream): every interval is (0, 0); offsets, given
// ranges and the first step's symbol are still checked.  One lane per pattern.
__global__ __launch_bounds__(FMX_BLOCK) void fmx_count_empty_p2_kernel(
    uint32_t max_character, uint32_t *status, const uint64_t *__restrict__ words, const uint64_t *__restrict__ off,
    uint64_t npat, const uint64_t *__restrict__ s0e0, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt) {
  const uint64_t ptot = npat ? off[npat] : 0;
  const uint64_t pmin = npat ? off[0] : 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < npat; k += stride) {
    const uint64_t a = off[k], b = off[k + 1];
    if (FMX_SPAN_BAD(a, b, pmin, ptot) || (s0e0 && (s0e0[2 * k] | s0e0[2 * k + 1]) != 0)) {
      atomicOr(status, 1u << FMX_ERR_ARG);
    } else if (b > a && ((uint32_t)(words[(b - 1u) >> 5] >> (2u * ((uint32_t)(b - 1u) & 31u))) & 3u) + 1u > max_character) {
      atomicOr(status, 1u << FMX_ERR_SYMBOL_RANGE);    // the first step's cs[c]
    }
    if (out_s) out_s[k] = 0;
    if (out_e) out_e[k] = 0;
    if (out_cnt) out_cnt[k] = 0;
  }
}

// ---- launch: the two rungs of fmx_route() that read u8 DNA-like FM indexes on the 32-bit engine ----
// which kernel serves the handle, if any: FMX_SHAPE_PAIR, FMX_SHAPE_F3, or FMX_SHAPE_GROUP for "none" (an index of an
// empty text has no records to route by: it is served when its alphabet is one a 3-bit level holds)
static inline FmxRoute fmx_packed2_route(const fmx_index *idx, const FmxDev &dv) {
  FmxRoute r = fmx_route(idx, dv, fmx_tune(), FMX_SHAPE_PAIR | FMX_SHAPE_F3 | FMX_HAS_KMER);
  const bool dna = !idx->is_wide && idx->kind == FMX_KIND_FM && idx->sym_bytes == 1 && idx->sym_bytes_abi == 1;
  if (dna && idx->n == 0 && idx->max_character <= 7) r.shape = FMX_SHAPE_F3;
  if (!dna || (r.shape != FMX_SHAPE_PAIR && r.shape != FMX_SHAPE_F3)) r.shape = FMX_SHAPE_GROUP;
  // the pair kernel takes every code for a symbol of the index: an alphabet of fewer than four symbols steps singly
  if (r.shape == FMX_SHAPE_PAIR && (dv.max_character != 4 || (r.km && dv.kmer_bits != 2))) r.shape = FMX_SHAPE_F3;
  return r;
}
bool fmx_packed2_served(const fmx_index *idx) { return fmx_packed2_route(idx, idx->dev).shape != FMX_SHAPE_GROUP; }

int fmx_launch_count_packed2(const fmx_index *idx, const uint64_t *d_words, const uint64_t *d_off, uint64_t npat,
                             const uint64_t *d_s0e0, uint64_t *d_s, uint64_t *d_e, uint64_t *d_cnt, hipStream_t st) {
  const FmxDev dv = fmx_launch_dev(idx);
  const FmxRoute r = fmx_packed2_route(idx, dv);
  if (r.shape == FMX_SHAPE_GROUP) {
    fmx_set_error(FMX_ERR_UNSUPPORTED, "packed patterns need a one-level FM index over u8 symbols on the 32-bit engine");
    return FMX_ERR_UNSUPPORTED;
  }
  if (npat == 0) return FMX_OK;
  if (idx->n == 0) {                                   // no record of any structure may be probed
    hipLaunchKernelGGL(fmx_count_empty_p2_kernel, dim3(fmx_grid_for_groups((npat + 7) / 8)), dim3(FMX_BLOCK), 0, st,
                       dv.max_character, dv.status, d_words, d_off, npat, d_s0e0, d_s, d_e, d_cnt);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
  fmx_time_begin(idx, st);
  uint64_t *steps = idx->timing == 1 ? idx->d_steps : nullptr;
  const dim3 grid(fmx_grid_for_groups(npat)), block(FMX_BLOCK);
  if (r.shape == FMX_SHAPE_PAIR) {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_count_pair_p2_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.pair_rec, dv.n,
                         dv.pair_row0, dv.pair_row1, dv.status, dv.kmer, dv.kmer_k, d_words, d_off, npat, d_s0e0, d_s,
                         d_e, d_cnt, steps);
    });
  } else {
    fmx_route_km(r, [&](auto km) {
      hipLaunchKernelGGL(fmx_count_f3_p2_kernel<km()>, grid, block, 0, st, dv.bw.lv[0].rec, dv.n, dv.max_character,
                         dv.status, dv.kmer, dv.kmer_k, dv.kmer_bits, d_words, d_off, npat, d_s0e0, d_s, d_e, d_cnt,
                         steps);
    });
  }
  fmx_time_end(idx, st);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
