// Inflate of one zlib stream (RFC 1950 / 1951) by one wave: the bit reader, the table builder and
// the symbol loop of rsx_dng_deflate.hip.  Everything here also compiles as host C++: the wave is a
// policy `W` -- 64 lanes on the device, one lane on the host (rsx_inflate_host.cpp) -- so the loop
// that meets damaged input runs on the CPU, under sanitizers, before it runs on a card.
//
// The control flow is wave-uniform: the bit buffer, the positions and every decoded symbol are the
// same in all lanes (w.uni() says so to the compiler, which keeps them in scalar registers).  The
// lanes differ only where bytes move: the fill of the tables, match and stored copies, the flush of
// the window and the Adler-32 over what is flushed.
//
// What W provides:
//   W::N, w.lane          lanes of the wave, this lane
//   w.uni(x)              x, known to be the same in all lanes
//   w.sync()              what the lanes wrote to `Shared` so far is visible to all of them
//   w.ballot(p)           bit l = p of lane l;  w.lt_mask(): the bits of the lanes below this one
//   w.reduce_add(x)       sum over the lanes (64-bit)
//   w.word(i)             the 32-bit little-endian word i of the input from its 4-byte-aligned base,
//                         zero behind the input; w.skip: bytes between that base and the stream
//   w.byte(i)             byte i of the stream (i < in_bytes)
//   w.store16(dst, v)     16 bytes to dst (16-byte aligned on the device)
//
// Safety: every table look-up is masked to the table, every read is behind in_bytes only as zeros
// and ends the stream (`used > total`), every write is checked against dst_len, every distance
// against the bytes produced, and every loop consumes at least one bit or produces one byte.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RSX_INF_FN __host__ __device__ __forceinline__
#else
#define RSX_INF_FN inline
#endif

namespace rsx_inflate {

enum Verdict : int { V_OK = 0, V_SHORT = 1, V_FAIL = 2 };

constexpr uint32_t RING = 32768, RING_MASK = RING - 1;
constexpr uint32_t LEN_ROOT = 9, DIST_ROOT = 6, CL_ROOT = 7;
// zlib's bounds for a root table of 9 resp. 6 bits plus sub-tables (852, 592)
constexpr uint32_t LEN_CAP = 852, DIST_CAP = 592, CL_CAP = 128;
constexpr uint32_t MAX_SYMS = 320; // 288 + 32 (fixed), 286 + 30 (dynamic)

// A table entry: bits to drop | kind << 4 | extra bits << 8 | value << 16.
//   K_LIT   a literal (value), or a code length symbol
//   K_BASE  a length or a distance: value + `extra` more bits
//   K_EOB   end of block
//   K_BAD   no such code (an incomplete set's hole, 286/287, distance codes 30/31)
//   K_LINK  root entry of a sub-table: value = its first entry, extra = its index bits
enum : uint32_t { K_LIT = 0, K_BASE = 1, K_EOB = 2, K_BAD = 3, K_LINK = 4 };
RSX_INF_FN uint32_t mk(uint32_t len, uint32_t kind, uint32_t extra, uint32_t val) {
  return len | (kind << 4) | (extra << 8) | (val << 16);
}
RSX_INF_FN uint32_t e_len(uint32_t e) { return e & 15u; }
RSX_INF_FN uint32_t e_kind(uint32_t e) { return (e >> 4) & 15u; }
RSX_INF_FN uint32_t e_extra(uint32_t e) { return (e >> 8) & 15u; }
RSX_INF_FN uint32_t e_val(uint32_t e) { return e >> 16; }

struct alignas(16) U4 {
  uint32_t x, y, z, w;
};

// What one stream's decoder keeps: LDS on the device (40 112 bytes, four waves in a CU's 160 KiB).
struct alignas(16) Shared {
  uint8_t ring[RING]; // the last 32 KiB of output; flushed in 16-byte pieces
  uint32_t lentab[LEN_CAP];
  uint32_t disttab[DIST_CAP];
  uint32_t cltab[CL_CAP];
  uint16_t work[MAX_SYMS]; // the symbols sorted by code length
  uint16_t count[16], first[16], offs[16];
  uint8_t lens[MAX_SYMS];
};

enum TableType : int { T_CODES = 0, T_LENS = 1, T_DISTS = 2 };

RSX_INF_FN uint32_t bitrev(uint32_t v, uint32_t n) { // the low n <= 16 bits of v, reversed
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
  return v >> (16u - n);
}

RSX_INF_FN uint32_t symbol_entry(int type, uint32_t sym, uint32_t len) {
  if (type == T_CODES)
    return mk(len, K_LIT, 0, sym);
  if (type == T_LENS) {
    if (sym < 256u)
      return mk(len, K_LIT, 0, sym);
    if (sym == 256u)
      return mk(len, K_EOB, 0, 0);
    if (sym < 265u)
      return mk(len, K_BASE, 0, sym - 254u);
    if (sym < 285u) {
      const uint32_t e = (sym - 261u) >> 2;
      return mk(len, K_BASE, e, ((4u + ((sym - 261u) & 3u)) << e) + 3u);
    }
    if (sym == 285u)
      return mk(len, K_BASE, 0, 258u);
    return mk(len, K_BAD, 0, 0); // 286, 287
  }
  if (sym < 4u)
    return mk(len, K_BASE, 0, sym + 1u);
  if (sym < 30u) {
    const uint32_t e = (sym >> 1) - 1u;
    return mk(len, K_BASE, e, ((2u + (sym & 1u)) << e) + 1u);
  }
  return mk(len, K_BAD, 0, 0); // 30, 31
}

// The decoding table of the n code lengths S.lens[off ..]: a root table of `root` bits, then the
// sub-tables of the longer codes, sized as inflate_table sizes them.  Accepts and rejects as
// inflate_table does: no code at all is a table of holes (T_CODES: rejected, its use could only
// fail later); an over-subscribed set is rejected; an incomplete one too, unless it is one code
// of one bit in a literal/length or a distance set.  false: rejected.
template <class W>
RSX_INF_FN bool build_table(W& w, Shared& S, uint32_t* tab, uint32_t cap, uint32_t root, int type,
                            uint32_t off, uint32_t n) {
  uint32_t cnt[16];
#pragma unroll
  for (int l = 0; l < 16; ++l)
    cnt[l] = 0;
  for (uint32_t base = 0; base < n; base += W::N) {
    const uint32_t i = base + w.lane;
    const uint32_t L = i < n ? S.lens[off + i] : 0u;
#pragma unroll
    for (int l = 1; l < 16; ++l)
      cnt[l] += uint32_t(__builtin_popcountll(w.ballot(L == uint32_t(l))));
  }
  uint32_t max = 0, total = 0;
  int32_t left = 1;
  bool over = false;
#pragma unroll
  for (int l = 1; l < 16; ++l) {
    if (cnt[l])
      max = uint32_t(l);
    total += cnt[l];
    left = left * 2 - int32_t(cnt[l]);
    if (left < 0)
      over = true;
  }
  const uint32_t root_size = 1u << root;
  if (max == 0) {
    if (type == T_CODES)
      return false;
    for (uint32_t k = w.lane; k < root_size; k += W::N)
      tab[k] = mk(1, K_BAD, 0, 0);
    w.sync();
    return true;
  }
  if (over)
    return false;
  if (left > 0 && (type == T_CODES || max != 1))
    return false;
  // first code and first sorted position of every length
  uint32_t fst[16], pos[16];
  {
    uint32_t code = 0, at = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
      fst[l] = code;
      pos[l] = at;
      code = (code + cnt[l]) << 1;
      at += cnt[l];
    }
  }
  if (w.lane == 0) {
#pragma unroll
    for (int l = 1; l < 16; ++l) {
      S.count[l] = uint16_t(cnt[l]);
      S.first[l] = uint16_t(fst[l]);
      S.offs[l] = uint16_t(pos[l]);
    }
  }
  // the symbols in the order of their codes: by length, then by symbol
  {
    uint32_t run[16];
#pragma unroll
    for (int l = 1; l < 16; ++l)
      run[l] = pos[l];
    for (uint32_t base = 0; base < n; base += W::N) {
      const uint32_t i = base + w.lane;
      const uint32_t L = i < n ? S.lens[off + i] : 0u;
#pragma unroll
      for (int l = 1; l < 16; ++l) {
        const uint64_t m = w.ballot(L == uint32_t(l));
        if (L == uint32_t(l))
          S.work[run[l] + uint32_t(__builtin_popcountll(m & w.lt_mask()))] = uint16_t(i);
        run[l] += uint32_t(__builtin_popcountll(m));
      }
    }
  }
  if (left > 0) // (one code of one bit: the other half of the table is a hole)
    for (uint32_t k = w.lane; k < root_size; k += W::N)
      tab[k] = mk(1, K_BAD, 0, 0);
  w.sync();
  // codes of up to `root` bits: a lane a code, repeated through the root table
  uint32_t n_short = 0;
#pragma unroll
  for (int l = 1; l < 16; ++l)
    if (uint32_t(l) <= root)
      n_short += cnt[l];
  for (uint32_t i = w.lane; i < n_short; i += W::N) {
    const uint32_t sym = S.work[i];
    const uint32_t L = S.lens[off + sym];
    const uint32_t code = uint32_t(S.first[L]) + (i - uint32_t(S.offs[L]));
    const uint32_t e = symbol_entry(type, sym, L);
    for (uint32_t k = bitrev(code, L); k < root_size; k += 1u << L)
      tab[k] = e;
  }
  // the longer ones, in code order: codes that share their first `root` bits share a sub-table
  uint32_t next = root_size, prefix = ~0u, sub_off = 0, sub_bits = 0;
  for (uint32_t i = n_short; i < total; ++i) {
    const uint32_t sym = w.uni(uint32_t(S.work[i]));
    const uint32_t L = w.uni(uint32_t(S.lens[off + sym]));
    const uint32_t idx = i - w.uni(uint32_t(S.offs[L]));
    const uint32_t code = w.uni(uint32_t(S.first[L])) + idx;
    const uint32_t drop = L - root;
    if ((code >> drop) != prefix) {
      prefix = code >> drop;
      // (inflate_table: as many bits as complete the sub-table from the codes still to come)
      uint32_t curr = drop;
      int32_t room = int32_t(1u << curr) - int32_t(w.uni(uint32_t(S.count[L])) - idx);
      while (curr + root < max && room > 0) {
        ++curr;
        room = room * 2 - int32_t(w.uni(uint32_t(S.count[curr + root])));
      }
      if (next + (1u << curr) > cap)
        return false;
      sub_off = next;
      sub_bits = curr;
      next += 1u << curr;
      for (uint32_t k = w.lane; k < (1u << curr); k += W::N)
        tab[sub_off + k] = mk(1, K_BAD, 0, 0);
      if (w.lane == 0)
        tab[bitrev(prefix, root)] = mk(root, K_LINK, curr, sub_off);
      w.sync();
    }
    if (drop > sub_bits)
      return false;
    const uint32_t e = symbol_entry(type, sym, drop);
    const uint32_t r = bitrev(code, L) >> root;
    for (uint32_t k = r + (w.lane << drop); k < (1u << sub_bits); k += W::N << drop)
      tab[sub_off + k] = e;
  }
  w.sync();
  return true;
}

// The LSB-first bit buffer over w.word(): up to 64 bits in `hold`; `used` counts what the stream
// has given, `total` is what it has.
template <class W>
struct Bits {
  uint64_t hold = 0, used = 0, total = 0;
  uint32_t nbits = 0, wi = 0;
  RSX_INF_FN void seek_byte(W& w, uint64_t byte) {
    const uint64_t bit = (uint64_t(w.skip) + byte) * 8u;
    wi = uint32_t(bit >> 5);
    hold = 0;
    nbits = 0;
    refill(w);
    hold >>= uint32_t(bit & 31u);
    nbits -= uint32_t(bit & 31u);
    used = byte * 8u;
    refill(w);
  }
  // at least 32 bits behind this
  RSX_INF_FN void refill(W& w) {
    if (nbits <= 32u) {
      hold |= uint64_t(w.word(wi)) << nbits;
      ++wi;
      nbits += 32u;
    }
  }
  RSX_INF_FN uint32_t peek(uint32_t n) const { return uint32_t(hold & ((uint64_t(1) << n) - 1u)); }
  RSX_INF_FN void drop(uint32_t n) {
    hold >>= n;
    nbits -= n;
    used += n;
  }
  RSX_INF_FN uint32_t take(uint32_t n) {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  RSX_INF_FN bool overrun() const { return used > total; }
};

// The window's bytes [flushed, upto) go out, and into the Adler-32 (a, b); `upto` is a multiple
// of 16 but for the last flush of a stream.
template <class W>
RSX_INF_FN void flush(W& w, Shared& S, uint8_t* out, uint32_t flushed, uint32_t upto, uint32_t& a,
                      uint32_t& b) {
  const uint32_t n = upto - flushed;
  if (n == 0)
    return;
  w.sync();
  uint64_t sum = 0, weighted = 0;
  for (uint32_t o = flushed + 16u * w.lane; o < upto; o += 16u * W::N) {
    const uint32_t cnt = upto - o < 16u ? upto - o : 16u;
    const U4 v = *reinterpret_cast<const U4*>(&S.ring[o & RING_MASK]);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    if (cnt == 16u) {
      w.store16(out + o, v);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16u; ++j)
        if (j < cnt)
          out[o + j] = uint8_t(q[j >> 2] >> (8u * (j & 3u)));
    }
    uint32_t s = 0, ws = 0; // (16 bytes: below 2^13 and 2^17)
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
      const uint32_t byte = j < cnt ? (q[j >> 2] >> (8u * (j & 3u))) & 255u : 0u;
      s += byte;
      ws += (16u - j) * byte;
    }
    // byte j of this piece counts n - (o - flushed) - j times
    sum += s;
    // (n - ... - 16 is below zero in the last, partial piece: the sum is right modulo 2^64)
    weighted += uint64_t(ws) + (uint64_t(n) - (o - flushed) - 16u) * uint64_t(s);
  }
  sum = w.reduce_add(sum);
  weighted = w.reduce_add(weighted);
  b = uint32_t((uint64_t(b) + uint64_t(n) * a + weighted) % 65521u);
  a = uint32_t((uint64_t(a) + sum) % 65521u);
  w.sync();
}

// One zlib stream into out[0 .. dst_len).  V_OK: the stream is whole, its Adler-32 right and it
// gave exactly dst_len bytes, all of them in `out`; V_SHORT: whole and right, fewer bytes (`out`
// is then not complete); V_FAIL: everything else.  *consumed: the stream's length up to and
// including the Adler-32 (not for V_FAIL); *produced: the bytes it gave.
template <class W>
RSX_INF_FN int inflate_stream(W& w, Shared& S, uint32_t in_bytes, uint8_t* out, uint32_t dst_len,
                              uint32_t* produced, uint32_t* consumed) {
  Bits<W> B;
  B.total = uint64_t(in_bytes) * 8u;
  B.seek_byte(w, 0);
  uint32_t pos = 0, flushed = 0, ad_a = 1, ad_b = 0;
  *produced = 0;
  *consumed = 0;
  {
    const uint32_t cmf = B.take(8), flg = B.take(8);
    if (B.overrun())
      return V_FAIL;
    if (((cmf << 8) | flg) % 31u != 0 || (cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u))
      return V_FAIL;
  }
  for (;;) {
    B.refill(w);
    const uint32_t last = B.take(1), btype = B.take(2);
    if (B.overrun())
      return V_FAIL;
    if (btype == 0) {
      // stored: to the byte boundary, LEN, NLEN, the bytes
      B.drop(uint32_t((8u - (B.used & 7u)) & 7u));
      B.refill(w);
      const uint32_t v = B.take(32);
      if (B.overrun())
        return V_FAIL;
      uint32_t len = v & 0xFFFFu;
      if (len != ((v >> 16) ^ 0xFFFFu))
        return V_FAIL;
      uint64_t at = B.used >> 3;
      if (len > uint64_t(in_bytes) - at || len > dst_len - pos)
        return V_FAIL;
      while (len) {
        const uint32_t c = len < 8192u ? len : 8192u;
        if (pos + c - flushed > RING) {
          flush(w, S, out, flushed, pos & ~15u, ad_a, ad_b);
          flushed = pos & ~15u;
        }
        for (uint32_t i = w.lane; i < c; i += W::N)
          S.ring[(pos + i) & RING_MASK] = w.byte(at + i);
        pos += c;
        at += c;
        len -= c;
      }
      w.sync();
      B.seek_byte(w, at);
    } else if (btype == 3) {
      return V_FAIL;
    } else {
      if (btype == 1) {
        for (uint32_t i = w.lane; i < MAX_SYMS; i += W::N)
          S.lens[i] = uint8_t(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : i < 288u ? 8 : 5);
        w.sync();
        if (!build_table(w, S, S.lentab, LEN_CAP, LEN_ROOT, T_LENS, 0, 288) ||
            !build_table(w, S, S.disttab, DIST_CAP, DIST_ROOT, T_DISTS, 288, 32))
          return V_FAIL;
      } else {
        const uint32_t nlen = B.take(5) + 257u, ndist = B.take(5) + 1u, ncode = B.take(4) + 4u;
        if (B.overrun() || nlen > 286u || ndist > 30u)
          return V_FAIL;
        if (w.lane < 19u)
          S.lens[w.lane] = 0;
        if (W::N < 19u)
          for (uint32_t i = 0; i < 19u; ++i)
            S.lens[i] = 0;
        w.sync();
        // the code length code's lengths come in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const uint64_t order_lo = 16u | (17u << 5) | (18u << 10) | (0u << 15) | (8u << 20) | (7u << 25) |
                                  (uint64_t(9) << 30) | (uint64_t(6) << 35) | (uint64_t(10) << 40) |
                                  (uint64_t(5) << 45) | (uint64_t(11) << 50) | (uint64_t(4) << 55);
        const uint64_t order_hi = 12u | (3u << 5) | (13u << 10) | (2u << 15) | (14u << 20) | (1u << 25) |
                                  (uint64_t(15) << 30);
        for (uint32_t i = 0; i < ncode; ++i) {
          B.refill(w);
          const uint32_t l = B.take(3);
          const uint32_t sym = uint32_t((i < 12u ? order_lo >> (5u * i) : order_hi >> (5u * (i - 12u))) & 31u);
          if (w.lane == 0)
            S.lens[sym] = uint8_t(l);
        }
        if (B.overrun())
          return V_FAIL;
        w.sync();
        if (!build_table(w, S, S.cltab, CL_CAP, CL_ROOT, T_CODES, 0, 19))
          return V_FAIL;
        // the literal/length and the distance lengths, as one sequence (a repeat may cross over)
        uint32_t have = 0, prev = 0;
        while (have < nlen + ndist) {
          B.refill(w);
          const uint32_t e = w.uni(S.cltab[B.peek(CL_ROOT)]);
          if (e_kind(e) != K_LIT)
            return V_FAIL;
          B.drop(e_len(e));
          const uint32_t sym = e_val(e);
          if (sym < 16u) {
            if (w.lane == 0)
              S.lens[have] = uint8_t(sym);
            ++have;
            prev = sym;
          } else {
            uint32_t rep, val = 0;
            if (sym == 16u) {
              if (have == 0)
                return V_FAIL;
              val = prev;
              rep = 3u + B.take(2);
            } else if (sym == 17u) {
              rep = 3u + B.take(3);
            } else {
              rep = 11u + B.take(7);
            }
            if (have + rep > nlen + ndist)
              return V_FAIL;
            for (uint32_t i = w.lane; i < rep; i += W::N)
              S.lens[have + i] = uint8_t(val);
            have += rep;
            prev = val;
          }
          if (B.overrun())
            return V_FAIL;
        }
        w.sync();
        if (w.uni(uint32_t(S.lens[256])) == 0)
          return V_FAIL; // no end-of-block code
        if (!build_table(w, S, S.lentab, LEN_CAP, LEN_ROOT, T_LENS, 0, nlen) ||
            !build_table(w, S, S.disttab, DIST_CAP, DIST_ROOT, T_DISTS, nlen, ndist))
          return V_FAIL;
      }
      // the symbols of the block
      for (;;) {
        if (B.overrun())
          return V_FAIL;
        if (pos + 258u - flushed > RING) {
          flush(w, S, out, flushed, pos & ~15u, ad_a, ad_b);
          flushed = pos & ~15u;
        }
        B.refill(w);
        uint32_t e = w.uni(S.lentab[B.peek(LEN_ROOT)]);
        if (e_kind(e) == K_LINK) {
          B.drop(LEN_ROOT);
          e = w.uni(S.lentab[(e_val(e) + B.peek(e_extra(e))) % LEN_CAP]);
        }
        B.drop(e_len(e));
        const uint32_t kind = e_kind(e);
        if (kind == K_LIT) {
          if (pos >= dst_len)
            return V_FAIL;
          if (w.lane == 0)
            S.ring[pos & RING_MASK] = uint8_t(e_val(e));
          ++pos;
          continue;
        }
        if (kind == K_EOB)
          break;
        if (kind != K_BASE)
          return V_FAIL;
        const uint32_t length = e_val(e) + B.take(e_extra(e));
        B.refill(w);
        uint32_t d = w.uni(S.disttab[B.peek(DIST_ROOT)]);
        if (e_kind(d) == K_LINK) {
          B.drop(DIST_ROOT);
          d = w.uni(S.disttab[(e_val(d) + B.peek(e_extra(d))) % DIST_CAP]);
        }
        B.drop(e_len(d));
        if (e_kind(d) != K_BASE)
          return V_FAIL;
        const uint32_t dist = e_val(d) + B.take(e_extra(d));
        if (B.overrun() || dist > pos || length > dst_len - pos)
          return V_FAIL;
        // the copy, by all lanes: every source byte lies in front of `pos`; a distance below the
        // length repeats its pattern
        w.sync();
        const uint32_t from = pos - dist;
        if (dist >= length) {
          for (uint32_t i = w.lane; i < length; i += W::N)
            S.ring[(pos + i) & RING_MASK] = S.ring[(from + i) & RING_MASK];
        } else if (dist == 1u) {
          const uint8_t v = S.ring[from & RING_MASK];
          for (uint32_t i = w.lane; i < length; i += W::N)
            S.ring[(pos + i) & RING_MASK] = v;
        } else {
          for (uint32_t i = w.lane; i < length; i += W::N)
            S.ring[(pos + i) & RING_MASK] = S.ring[(from + i % dist) & RING_MASK];
        }
        w.sync();
        pos += length;
      }
    }
    if (last)
      break;
  }
  // the Adler-32 of the output, most significant byte first, from the next byte boundary
  B.drop(uint32_t((8u - (B.used & 7u)) & 7u));
  B.refill(w);
  const uint32_t t = B.take(32);
  if (B.overrun())
    return V_FAIL;
  flush(w, S, out, flushed, pos, ad_a, ad_b);
  const uint32_t want = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);
  if (want != ((ad_b << 16) | ad_a))
    return V_FAIL;
  *produced = pos;
  *consumed = uint32_t(B.used >> 3);
  return pos == dst_len ? V_OK : V_SHORT;
}

} // namespace rsx_inflate
