// fmx_wide_suffix.h -- batched longest-suffix match on the 64-bit engine (included by fmx_wide.hip): the semantics and
// the monotonicity argument of fmx_suffix.h, one kernel per count kernel of fmx_wide.hip, same shapes.  `mc` is
// min_count with 0 already replaced by 1.
#pragma once

// one-level indexes, a group per pattern (the twin of fmxw_count_kernel)
template <bool LDSB, bool KM>
__global__ __launch_bounds__(FMXW_BLOCK) void fmxw_sfx_kernel(
    FmxWideDev w, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint64_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  FMXW_BASES(w, LDSB);
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = npat ? off[npat] : 0;       // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  for (uint64_t k = gid; k < npat; k += ngroups) {
    const uint64_t pbeg = off[k], pend = off[k + 1];
    uint64_t j = pend - pbeg, len = 0;
    // offsets that go backwards or leave the pattern buffer: refuse, do not read
    bool bad = FMX_SPAN_BAD(pbeg, pend, pmin, ptot);
    uint64_t s = 0, e = w.n;
    if (s0e0) {
      s = s0e0[2 * k];
      e = s0e0[2 * k + 1];
      bad |= s > w.n || e > w.n;                    // not a range of this index
    }
    if (bad) {
      if (g == 0) atomicOr(w.status, 1u << FMX_ERR_ARG);
      s = 0; e = 0; j = 0;
    } else if (e < s || e - s < mc) {               // a start pair below min_count: no step can pass
      j = 0;
    }
    if constexpr (KM) {
      if (!s0e0 && j >= w.kmer_k) {                 // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code(pat, pbeg + j, w.kmer_k, w.kmer_bits, w.max_character, g, code)) {
          FMX_CHECK(code < (1u << (w.kmer_bits * w.kmer_k)));
          FMX_TOUCH_G0N(g, &w.kmer[code]);
          const FmxWideKmer se = w.kmer[code];
          if (se.e - se.s >= mc) { s = se.s; e = se.e; j -= w.kmer_k; len = w.kmer_k; }
        }
      }
    }
    uint32_t c = j ? pat[pbeg + j - 1] : 0u;        // last symbol first
    while (j) {
      if (c > w.max_character) break;               // an absent symbol ends the match
      FMX_CHECK((e >> 8) < w.n / 256u + 1u && (s >> w.sb_shift) < w.nsb && (e >> w.sb_shift) < w.nsb);
      const uint4 pa = w.rec[(size_t)(s >> 8) * 8u + g], pb = w.rec[(size_t)(e >> 8) * 8u + g];
      const uint32_t cn = j > 1 ? pat[pbeg + j - 2] : 0u;      // rides along with the record loads
      const uint64_t ba = base_at(s, c), bb = base_at(e, c);
      const uint64_t ns = ba + fmx_group_sum(fmx_piece_rank<3>(pa, (uint32_t)s & 255u, c, g));
      const uint64_t ne = bb + fmx_group_sum(fmx_piece_rank<3>(pb, (uint32_t)e & 255u, c, g));
      if (ne - ns < mc) break;                      // keep the previous (s, e, len)
      s = ns; e = ne; len++;
      c = cn;
      j--;
    }
    if (g == 0) {
      if (out_s) out_s[k] = s;
      if (out_e) out_e[k] = e;
      if (out_cnt) out_cnt[k] = e >= s ? e - s : 0ull;   // (a given start pair with e < s holds no row)
      if (out_len) out_len[k] = len;
    }
  }
}

// one-level indexes with the pair index (the twin of fmxw_count_pair_kernel; the rules of fmx_sfx_pair_kernel)
template <bool LDSB, bool KM>
__global__ __launch_bounds__(FMXW_BLOCK) void fmxw_sfx_pair_kernel(
    FmxWideDev w, FmxWidePair pr, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint64_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  FMXW_BASES(w, LDSB);
  FMXW_PAIR_BASES(w, pr, LDSB);
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = npat ? off[npat] : 0;       // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  for (uint64_t k = gid; k < npat; k += ngroups) {
    const uint64_t pbeg = off[k], pend = off[k + 1];
    uint64_t j = pend - pbeg, len = 0;
    // offsets that go backwards or leave the pattern buffer: refuse, do not read
    bool bad = FMX_SPAN_BAD(pbeg, pend, pmin, ptot);
    uint64_t s = 0, e = w.n;
    if (s0e0) {
      s = s0e0[2 * k];
      e = s0e0[2 * k + 1];
      bad |= s > w.n || e > w.n;                    // not a range of this index
    }
    if (bad) {
      if (g == 0) atomicOr(w.status, 1u << FMX_ERR_ARG);
      s = 0; e = 0; j = 0;
    } else if (e < s || e - s < mc) {               // a start pair below min_count: no step can pass
      j = 0;
    }
    if constexpr (KM) {
      if (!s0e0 && j >= w.kmer_k) {                 // all kmer_k symbols at once when the entry is wide enough
        uint32_t code;
        if (fmx_kmer_code(pat, pbeg + j, w.kmer_k, w.kmer_bits, w.max_character, g, code)) {
          FMX_CHECK(code < (1u << (w.kmer_bits * w.kmer_k)));
          FMX_TOUCH_G0N(g, &w.kmer[code]);
          const FmxWideKmer se = w.kmer[code];
          if (se.e - se.s >= mc) { s = se.s; e = se.e; j -= w.kmer_k; len = w.kmer_k; }
        }
      }
    }
    uint32_t c2 = j ? pat[pbeg + j - 1] : 0u;       // c2 = last unread symbol, c1 = the one before it
    uint32_t c1 = j > 1 ? pat[pbeg + j - 2] : 0u;
    while (j) {
      if (c2 > w.max_character) break;              // an absent symbol ends the match
      const bool pair = j >= 2 && (c2 - 1u) < w.max_character && (c1 - 1u) < w.max_character;
      FMX_CHECK((s >> w.sb_shift) < w.nsb && (e >> w.sb_shift) < w.nsb);
      // the two symbols after these ride along with the record loads
      const uint32_t n1 = j > 2 ? pat[pbeg + j - 3] : 0u;
      const uint32_t n2 = j > 3 ? pat[pbeg + j - 4] : 0u;
      uint32_t used = 0;
      if (pair) {
        const uint32_t code = (c1 - 1u) * 4u + (c2 - 1u);
        FMX_CHECK((s >> 7) < w.n / 128u + 1u && (e >> 7) < w.n / 128u + 1u);
        FMX_TOUCH_G0(g, &pr.rec[(size_t)(s >> 7) * 8u]);
        if ((e >> 7) != (s >> 7)) FMX_TOUCH_G0(g, &pr.rec[(size_t)(e >> 7) * 8u]);
        const uint4 pa = pr.rec[(size_t)(s >> 7) * 8u + g], pb = pr.rec[(size_t)(e >> 7) * 8u + g];
        const uint64_t ba = pbase_at(s, code), bb = pbase_at(e, code);
        uint64_t ns = ba + fmx_group_sum(fmx_piece_rank<4>(pa, (uint32_t)s & 127u, code, g));
        uint64_t ne = bb + fmx_group_sum(fmx_piece_rank<4>(pb, (uint32_t)e & 127u, code, g));
        if (code == 0u) {                           // the two rows without a 2-gram are stored as code 0
          ns -= (uint64_t)(s > pr.row0) + (uint64_t)(s > pr.row1);
          ne -= (uint64_t)(e > pr.row0) + (uint64_t)(e > pr.row1);
        }
        if (ne - ns >= mc) { s = ns; e = ne; used = 2; }
      }
      if (used == 0) {                              // one symbol on the 1-gram records
        FMX_CHECK((e >> 8) < w.n / 256u + 1u && (s >> 8) < w.n / 256u + 1u);
        FMX_TOUCH_G0(g, &w.rec[(size_t)(s >> 8) * 8u]);
        if ((e >> 8) != (s >> 8)) FMX_TOUCH_G0(g, &w.rec[(size_t)(e >> 8) * 8u]);
        const uint4 qa = w.rec[(size_t)(s >> 8) * 8u + g], qb = w.rec[(size_t)(e >> 8) * 8u + g];
        const uint64_t s1 = base_at(s, c2) + fmx_group_sum(fmx_piece_rank<3>(qa, (uint32_t)s & 255u, c2, g));
        const uint64_t e1 = base_at(e, c2) + fmx_group_sum(fmx_piece_rank<3>(qb, (uint32_t)e & 255u, c2, g));
        if (e1 - s1 >= mc) { s = s1; e = e1; used = 1; }
        len += used;
        if (pair || used == 0) break;               // after a failed pair probe the second symbol is known to fail
      } else {
        len += 2;
      }
      j -= used;
      if (used == 2) { c2 = n1; c1 = n2; } else { c2 = c1; c1 = n1; }
    }
    if (g == 0) {
      if (out_s) out_s[k] = s;
      if (out_e) out_e[k] = e;
      if (out_cnt) out_cnt[k] = e >= s ? e - s : 0ull;   // (a given start pair with e < s holds no row)
      if (out_len) out_len[k] = len;
    }
  }
}

// generic indexes (FM, RLFM, multi-pieces), a group per pattern (the twin of fmxw_g_count_kernel; stepwise only)
template <bool GLDS, int KD>
__global__ __launch_bounds__(FMXW_BLOCK) void fmxw_g_sfx_kernel(
    FmxWideDev w, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint64_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  constexpr bool RL = KD == FMX_KIND_RLFM, MP = KD == FMX_KIND_MULTI;
  FMXW_GBASES(w, GLDS);
  const uint32_t g = threadIdx.x & (FMX_GROUP - 1);
  const uint64_t gid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FMX_GROUP;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / FMX_GROUP;
  const uint64_t ptot = npat ? off[npat] : 0;       // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  for (uint64_t k = gid; k < npat; k += ngroups) {
    const uint64_t pbeg = off[k], pend = off[k + 1];
    uint64_t j = pend - pbeg, len = 0;
    bool bad = FMX_SPAN_BAD(pbeg, pend, pmin, ptot);          // offsets that go backwards or leave the pattern buffer
    uint64_t s = 0, e = w.n;
    if (s0e0) {
      s = s0e0[2 * k];
      e = s0e0[2 * k + 1];
      bad |= s > w.n || e > w.n;                    // not a range of this index
    }
    if (bad) {                                      // refuse, do not read
      if (g == 0) atomicOr(w.status, 1u << FMX_ERR_ARG);
      s = 0; e = 0; j = 0;
    } else if (e < s || e - s < mc) {               // a start pair below min_count: no step can pass
      j = 0;
    }
    uint32_t c = j ? fmx_load_sym(pat, w.sym_bytes, pbeg + j - 1) : 0u;
    while (j) {
      if (c > w.max_character) break;               // an absent symbol ends the match
      uint32_t cn = 0;
      uint64_t ns = s, ne = e;
      if constexpr (RL) {
        if (j > 1) cn = fmx_load_sym(pat, w.sym_bytes, pbeg + j - 2);
        fmxw_r_lf_map2_pair(w, gbase, gk, c, ns, ne, g);
      } else {
        for (uint32_t l = 0; l < w.nlevels; l++) {
          const FmxWideLevel &L = w.lv[l];
          const uint32_t code = (c >> L.shift) & L.mask;
          const uint4 pa = fmxw_g_piece(L, ns, g), pb = fmxw_g_piece(L, ne, g);
          if (l == 0 && j > 1) cn = fmx_load_sym(pat, w.sym_bytes, pbeg + j - 2);             // rides along with the record loads
          const uint64_t ba = gbase(l, ns, code), bb = gbase(l, ne, code);
          ns = ba + fmxw_g_rank32(L, pa, ns, code, g);
          ne = bb + fmxw_g_rank32(L, pb, ne, code, g);
        }
        const uint64_t kc = gk(c);
        if (MP && c == 0u) {                        // multi_pieces.rs:147-153
          ns = fmxw_multi_zero(w, s, kc + ns);
          ne = fmxw_multi_zero(w, e, kc + ne);
        } else {
          ns += kc;
          ne += kc;
        }
      }
      // (ne < ns: lf_map2(0, .) of a multi-pieces index is not monotone, multi_pieces.rs:147-153 -- below every min_count)
      if (ne < ns || ne - ns < mc) break;           // keep the previous (s, e, len)
      s = ns; e = ne; len++;
      c = cn;
      j--;
    }
    if (g == 0) {
      if (out_s) out_s[k] = s;
      if (out_e) out_e[k] = e;
      if (out_cnt) out_cnt[k] = e >= s ? e - s : 0ull;   // (a given start pair with e < s holds no row)
      if (out_len) out_len[k] = len;
    }
  }
}

// generic indexes, an interval endpoint per lane (the twin of fmxw_g_count_ep_kernel; the rules of fmx_sfx_ep_kernel)
template <bool GLDS, int KD, bool KM>
__global__ __launch_bounds__(FMXW_BLOCK) void fmxw_g_sfx_ep_kernel(
    FmxWideDev w, const void *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
    const uint64_t *__restrict__ s0e0, uint64_t mc, uint64_t *__restrict__ out_s, uint64_t *__restrict__ out_e,
    uint64_t *__restrict__ out_cnt, uint64_t *__restrict__ out_len) {
  FMXW_GBASES(w, GLDS);
  const uint32_t lane = threadIdx.x & 63u, g = lane & 7u, base = lane & ~7u;
  const uint32_t is_e = g & 1u;
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) >> 3;
  const uint64_t slot = (uint64_t)(g >> 1) * ngroups + (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3);
  const uint64_t nslots = ngroups * 4u;
  const uint64_t ptot = npat ? off[npat] : 0;       // symbols the caller declares behind `pat`
  const uint64_t pmin = npat ? off[0] : 0;      // ... starting at this symbol (a slice of a larger batch keeps its absolute offsets)
  uint64_t k = slot, pbeg = 0, j = 0, pos = 0, len = 0;
  bool active = k < npat, fresh = true;
  uint32_t c = 0;
  while (__any(active)) {
    if (active && fresh) {                            // (both lanes of a pair are here together)
      pbeg = off[k];
      const uint64_t pend = off[k + 1];
      j = pend - pbeg;
      len = 0;
      bool bad = FMX_SPAN_BAD(pbeg, pend, pmin, ptot);          // offsets that go backwards or leave the pattern buffer
      uint64_t oth;                                   // the pair's other end
      if (s0e0) {
        const uint64_t mine = s0e0[2 * k + is_e], other = s0e0[2 * k + (is_e ^ 1u)];
        pos = mine;
        oth = other;
        bad |= mine > w.n || other > w.n;             // not a range of this index
      } else {
        pos = is_e ? w.n : 0ull;
        oth = is_e ? 0ull : w.n;
      }
      const uint64_t ss = is_e ? oth : pos, ee = is_e ? pos : oth;
      if (bad) {                                      // refuse, do not read
        if (is_e) atomicOr(w.status, 1u << FMX_ERR_ARG);
        pos = 0; j = 0;
      } else if (ee < ss || ee - ss < mc) {           // a start pair below min_count: no step can pass
        j = 0;
      }
      if constexpr (KM) {
        if (!s0e0 && j >= w.kmer_k) {                 // all kmer_k symbols at once when the entry is wide enough
          uint32_t code;
          if (fmx_kmer_code_lane((const uint8_t *)pat, pbeg + j, w.kmer_k, w.kmer_bits, w.max_character, code)) {
            FMX_CHECK(code < (1u << (w.kmer_bits * w.kmer_k)));
            FMX_TOUCH(&w.kmer[code]);
            const FmxWideKmer se = w.kmer[code];
            if (se.e - se.s >= mc) { pos = is_e ? se.e : se.s; j -= w.kmer_k; len = w.kmer_k; }
          }
        }
      }
      c = j ? fmx_load_sym(pat, w.sym_bytes, pbeg + j - 1) : 0u;
      fresh = false;
    }
    if (active && j != 0 && c > w.max_character) j = 0;   // an absent symbol ends the match
    const bool stepping = active && j != 0;
    const uint32_t cn = (stepping && j > 1) ? fmx_load_sym(pat, w.sym_bytes, pbeg + j - 2) : 0u;   // rides along with the probes
    uint64_t np;
    if constexpr (KD == FMX_KIND_RLFM) np = fmxw_r_ep_lf_map2(w, gbase, gk, stepping ? c : 0u, stepping ? pos : 0ull, stepping, base, g);
    else np = fmxw_g_ep_lf_map2<KD == FMX_KIND_MULTI>(w, gbase, gk, stepping ? c : 0u, stepping ? pos : 0ull, stepping, base, g);
    const uint64_t onp = (uint64_t)fmx_dpp_xor1((uint32_t)np) | ((uint64_t)fmx_dpp_xor1((uint32_t)(np >> 32)) << 32);
    if (stepping) {
      const uint64_t ns = is_e ? onp : np, ne = is_e ? np : onp;
      // (ne < ns: lf_map2(0, .) of a multi-pieces index is not monotone, multi_pieces.rs:147-153 -- below every min_count)
      if (ne < ns || ne - ns < mc) {
        j = 0;                                        // keep the previous endpoint and len
      } else {
        pos = np;
        len++;
        c = cn;
        j--;
      }
    }
    const uint64_t other = (uint64_t)fmx_dpp_xor1((uint32_t)pos) | ((uint64_t)fmx_dpp_xor1((uint32_t)(pos >> 32)) << 32);
    if (active && j == 0) {
      if (is_e) {
        if (out_e) out_e[k] = pos;
        if (out_cnt) out_cnt[k] = pos >= other ? pos - other : 0ull;   // (a given start pair with e < s holds no row)
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

// the dispatch of fmxw_launch_count, kernel for kernel
int fmxw_launch_suffix_match(const fmx_index *idx, const void *d_pat, const uint64_t *d_off, uint64_t npat,
                             const uint64_t *d_s0e0, uint64_t mc, uint64_t *d_s, uint64_t *d_e, uint64_t *d_cnt,
                             uint64_t *d_len, hipStream_t st) {
  if (npat == 0) return FMX_OK;
  if (mc == 0) mc = 1;
  const FmxWideDev w = fmxw_dev(idx);
  if (w.generic) {
#define FMXW_GSFX(GLDS, KD)                                                                                         \
  hipLaunchKernelGGL((fmxw_g_sfx_kernel<GLDS, KD>), dim3(fmxw_grid(npat)), dim3(FMXW_BLOCK), 0, st, w, d_pat, d_off,  \
                     npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len)
#define FMXW_RSFX(GLDS, KD)                                                                                         \
  do {                                                                                                              \
    if (w.kmer)                                                                                                     \
      hipLaunchKernelGGL((fmxw_g_sfx_ep_kernel<GLDS, KD, true>), dim3((unsigned)eb), dim3(FMXW_BLOCK), 0, st, w,     \
                         d_pat, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len);                                   \
    else                                                                                                            \
      hipLaunchKernelGGL((fmxw_g_sfx_ep_kernel<GLDS, KD, false>), dim3((unsigned)eb), dim3(FMXW_BLOCK), 0, st, w,    \
                         d_pat, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len);                                   \
  } while (0)
    const bool glds = w.nsb <= FMXW_GLDS_SB;
    if (w.sb_shift <= 31u && !fmxw_env_group()) {     // an interval endpoint per lane (32 patterns per block at a time)
      uint64_t eb = (npat + FMXW_BLOCK / 8 - 1) / (FMXW_BLOCK / 8);
      if (eb > FMXW_EP_BLOCKS) eb = FMXW_EP_BLOCKS;
      if (w.kind == FMX_KIND_RLFM) { if (glds) FMXW_RSFX(true, FMX_KIND_RLFM); else FMXW_RSFX(false, FMX_KIND_RLFM); }
      else if (w.kind == FMX_KIND_MULTI) { if (glds) FMXW_RSFX(true, FMX_KIND_MULTI); else FMXW_RSFX(false, FMX_KIND_MULTI); }
      else if (glds) FMXW_RSFX(true, FMX_KIND_FM); else FMXW_RSFX(false, FMX_KIND_FM);
    }
    else if (w.kind == FMX_KIND_RLFM) { if (glds) FMXW_GSFX(true, FMX_KIND_RLFM); else FMXW_GSFX(false, FMX_KIND_RLFM); }
    else if (w.kind == FMX_KIND_MULTI) { if (glds) FMXW_GSFX(true, FMX_KIND_MULTI); else FMXW_GSFX(false, FMX_KIND_MULTI); }
    else if (glds) FMXW_GSFX(true, FMX_KIND_FM); else FMXW_GSFX(false, FMX_KIND_FM);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }
#define FMXW_SFX(LDSB, KM)                                                                                          \
  hipLaunchKernelGGL((fmxw_sfx_kernel<LDSB, KM>), dim3(fmxw_grid(npat)), dim3(FMXW_BLOCK), 0, st, w,                  \
                     (const uint8_t *)d_pat, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len)
#define FMXW_PSFX(LDSB, KM)                                                                                         \
  hipLaunchKernelGGL((fmxw_sfx_pair_kernel<LDSB, KM>), dim3(fmxw_grid(npat)), dim3(FMXW_BLOCK), 0, st, w,             \
                     idx->wpair, (const uint8_t *)d_pat, d_off, npat, d_s0e0, mc, d_s, d_e, d_cnt, d_len)
  const bool ldsb = w.nsb <= FMXW_LDS_SB;
  if (idx->wpair.rec) {                                 // FMX_FLAG_PAIR_INDEX: two symbols per probe
    if (w.kmer) { if (ldsb) FMXW_PSFX(true, true); else FMXW_PSFX(false, true); }
    else if (ldsb) FMXW_PSFX(true, false); else FMXW_PSFX(false, false);
  }
  else if (w.kmer) { if (ldsb) FMXW_SFX(true, true); else FMXW_SFX(false, true); }
  else if (ldsb) FMXW_SFX(true, false); else FMXW_SFX(false, false);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}
