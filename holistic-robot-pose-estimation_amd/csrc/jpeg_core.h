// Baseline JPEG decoder core: bit reader, Huffman decode, block decode, libjpeg's "islow" inverse DCT, "fancy" chroma
// up-sampling and the YCbCr -> RGB step.  Plain inline functions, the same for the kernels of jpeg.hip and for a host compiler
// (tests/jpeg_host_check.cpp): JPEG_HD is the only thing that differs, and it is empty for a host compiler.
//
// Safety rules, held by tests/jpeg_host_check.cpp on damaged streams: every byte read is checked against the end of its
// segment; a stuffed FF 00 is one byte; a marker inside a segment, a code longer than 16 bits, a coefficient index >= 64 or
// running out of data ends the segment with a non-zero status and leaves the rest of its coefficients zero; a segment that
// decodes but is not used up to its padding bits gets HRP_JPEG_WARN_TRAILING; nothing outside
// the buffers that the descriptor names (checked by jpeg_image_fits / jpeg_segment_fits) is read or written.
// All arithmetic that a damaged stream can drive out of range wraps (uint32_t) or is cast down explicitly: no undefined behaviour.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/hrp.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_HD inline
#define JPEG_UNROLL
#endif

namespace jpeg {

// ---- geometry ---------------------------------------------------------------------------------------------------------------
struct Geom {
  int mcux, mcuy;        // MCUs per row / column
  int bw[3], bh[3];      // blocks per row / column of each component plane (whole MCUs)
  int base[3];           // first block of each component (blocks of one image: component 0 raster, then 1, then 2)
  int blocks;            // all blocks of the image
  int cw, ch;            // real (down-sampled) chroma columns / rows
};

JPEG_HD bool jpeg_geom(const hrp_jpeg_image& d, Geom& g) {
  const bool samp = (d.hsamp == 1 && d.vsamp == 1) || (d.hsamp == 2 && (d.vsamp == 1 || d.vsamp == 2));
  if (!samp || d.width < 1 || d.height < 1 || d.width > 16384 || d.height > 16384) return false;
  g.mcux = (d.width + 8 * d.hsamp - 1) / (8 * d.hsamp);
  g.mcuy = (d.height + 8 * d.vsamp - 1) / (8 * d.vsamp);
  g.bw[0] = g.mcux * d.hsamp;
  g.bh[0] = g.mcuy * d.vsamp;
  g.bw[1] = g.bw[2] = g.mcux;
  g.bh[1] = g.bh[2] = g.mcuy;
  g.base[0] = 0;
  g.base[1] = g.bw[0] * g.bh[0];
  g.base[2] = g.base[1] + g.mcux * g.mcuy;
  g.blocks = g.base[2] + g.mcux * g.mcuy;
  g.cw = (d.width + d.hsamp - 1) / d.hsamp;
  g.ch = (d.height + d.vsamp - 1) / d.vsamp;
  return true;
}

// the descriptor against the buffers of the call: true when everything the image names lies inside them
JPEG_HD bool jpeg_image_fits(const hrp_jpeg_image& d, Geom& g, size_t nbytes, size_t ncoef, size_t nplanes, size_t nframes) {
  if (!jpeg_geom(d, g)) return false;
  if (d.hsamp == 2 && g.cw <= 2) return false;      // libjpeg replicates instead of filtering there: not built
  if (d.restart_interval < 0) return false;
  for (int c = 0; c < 3; ++c)
    if (d.comp_tq[c] > 3 || d.comp_td[c] > 1 || d.comp_ta[c] > 1) return false;
  const uint64_t n = 64ull * (uint64_t)g.blocks, fb = 3ull * (uint64_t)d.width * (uint64_t)d.height;
  if (d.scan_off < 0 || d.scan_len < 0 || (uint64_t)d.scan_off > nbytes || (uint64_t)d.scan_len > nbytes - (uint64_t)d.scan_off) return false;
  if (d.sum_len < d.scan_len || (uint64_t)d.sum_len > nbytes - (uint64_t)d.scan_off) return false;
  if (d.coef_off < 0 || (d.coef_off & 63) || (uint64_t)d.coef_off > ncoef || n > ncoef - (uint64_t)d.coef_off) return false;
  if (d.plane_off < 0 || (uint64_t)d.plane_off > nplanes || n > nplanes - (uint64_t)d.plane_off) return false;
  if (d.frame_off < 0 || (uint64_t)d.frame_off > nframes || fb > nframes - (uint64_t)d.frame_off) return false;
  return true;
}

JPEG_HD bool jpeg_segment_fits(const hrp_jpeg_segment& s, const hrp_jpeg_image& d, const Geom& g) {
  if (s.off < d.scan_off || s.len < 0 || s.off > d.scan_off + d.scan_len || s.len > d.scan_off + d.scan_len - s.off) return false;
  if (s.mcu0 < 0 || s.mcu0 >= g.mcux * g.mcuy) return false;
  return d.restart_interval == 0 ? s.mcu0 == 0 : s.mcu0 % d.restart_interval == 0;
}

// ---- checksum ------------------------------------------------------------------------------------------------------------------
// zlib's Adler-32 of p[0, n) in a form that splits over lanes: a = 1 + sum d_i, b = n + sum (n - i) d_i, both mod 65521.
// jpeg_adler_part gives the two sums over [lo, hi) (already reduced), jpeg_adler_finish the checksum from the sums of all parts.
// A change of one byte changes a by less than 65521 and so always changes the checksum.
JPEG_HD void jpeg_adler_part(const uint8_t* p, size_t n, size_t lo, size_t hi, uint32_t& a, uint32_t& b) {
  uint64_t sa = 0, sb = 0;
  uint32_t w = (uint32_t)((n - lo) % 65521u);      // (n - i) mod 65521, counted down with the index
  for (size_t i = lo; i < hi; ++i) {
    sa += p[i];
    sb += (uint64_t)w * p[i];
    w = w ? w - 1 : 65520u;
    if ((i & 0xFFFF) == 0xFFFF) sb %= 65521u;      // 2^16 terms below 2^24 each between reductions
  }
  a = (uint32_t)(sa % 65521u);
  b = (uint32_t)(sb % 65521u);
}

JPEG_HD uint32_t jpeg_adler_finish(size_t n, uint64_t a_sum, uint64_t b_sum) {
  return (uint32_t)(((n % 65521u + b_sum) % 65521u) << 16) | (uint32_t)((1 + a_sum) % 65521u);
}

// ---- Huffman tables ------------------------------------------------------------------------------------------------------------
// Canonical decode without a per-code table: with the next 16 bits of the stream as a number p, the code has the smallest
// length l with p < limit[l] (the first code after those of length l, left-aligned), and its symbol is values[(p >> (16 - l)) +
// offset[l]].  limit[] never decreases, so l is one more than the number of limits that p has reached: sixteen independent
// compares instead of a loop whose every step waits for a load.
struct Lut {
  int32_t limit[20];      // [1..16] used; [17] = INT32_MAX closes the count; padded to whole 16-byte rows
  int32_t offset[20];
  uint8_t values[256];
};
// what one decoding lane keeps at hand (LDS on the device, the stack on the host)
struct Tables {
  Lut lut[4];             // DC 0, DC 1, AC 0, AC 1
  uint8_t natural[64];    // zig-zag position -> natural (row-major) index
};

JPEG_HD bool jpeg_build_lut(const hrp_jpeg_huff& h, Lut& t) {
  int32_t code = 0, k = 0;
  bool ok = true;
  t.limit[0] = 0;
  t.offset[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int32_t n = h.counts[l - 1];
    t.offset[l] = k - code;
    k += n;
    code += n;
    if (code > (1 << l)) ok = false;
    t.limit[l] = code << (16 - l);
    code <<= 1;
  }
  if (k > 256) ok = false;
  t.limit[17] = t.limit[18] = t.limit[19] = INT32_MAX;
  t.offset[17] = t.offset[18] = t.offset[19] = 0;
  for (int i = 0; i < 256; ++i) t.values[i] = h.values[i];
  return ok;
}

JPEG_HD bool jpeg_build_tables(const hrp_jpeg_image& d, Tables& t) {
  const uint8_t natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  for (int i = 0; i < 64; ++i) t.natural[i] = natural[i];
  return jpeg_build_lut(d.dc[0], t.lut[0]) & jpeg_build_lut(d.dc[1], t.lut[1]) & jpeg_build_lut(d.ac[0], t.lut[2]) &
         jpeg_build_lut(d.ac[1], t.lut[3]);
}

// ---- bit reader ----------------------------------------------------------------------------------------------------------------
// Past the end of the segment (or at a marker) the reader feeds zero bits and counts them; consuming one of those sets err.
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc;     // the low n bits are unread, most significant first
  int n, fake;      // fake: how many of them (the lowest) are not from the stream
  int stop;         // HRP_JPEG_ERR_DATA / _MARKER once the stream has ended, else 0
  int err;
};

JPEG_HD void bits_open(Bits& b, const uint8_t* p, size_t len) {
  b.p = p;
  b.end = p + len;
  b.acc = 0;
  b.n = b.fake = b.stop = b.err = 0;
}

// called with n <= 32: four bytes at once when none of them is FF, else byte by byte
JPEG_HD void bits_fill(Bits& b) {
  if (!b.stop && b.end - b.p >= 4) {
    uint32_t w;
    __builtin_memcpy(&w, b.p, 4);
    const uint32_t x = ~w;
    if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {      // no byte of x is zero: no FF in w
      w = (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24);
      b.acc = (b.acc << 32) | w;
      b.n += 32;
      b.p += 4;
      return;
    }
  }
  while (b.n <= 56) {
    uint32_t v = 0;
    if (!b.stop) {
      if (b.p >= b.end) {
        b.stop = HRP_JPEG_ERR_DATA;
      } else {
        v = *b.p;
        if (v != 0xFF) {
          ++b.p;
        } else if (b.end - b.p < 2) {      // FF as the last byte: neither a stuffed byte nor a marker
          b.stop = HRP_JPEG_ERR_DATA;
          v = 0;
        } else if (b.p[1] == 0) {
          b.p += 2;
        } else {
          b.stop = HRP_JPEG_ERR_MARKER;
          v = 0;
        }
      }
    }
    if (b.stop) b.fake += 8;
    b.acc = (b.acc << 8) | v;
    b.n += 8;
  }
}

JPEG_HD uint32_t bits_peek16(Bits& b) {
  if (b.n <= 32) bits_fill(b);
  return (uint32_t)(b.acc >> (b.n - 16)) & 0xFFFFu;
}

JPEG_HD void bits_skip(Bits& b, int k) {
  b.n -= k;
  if (b.n < b.fake) {
    b.err |= b.stop;
    b.fake = b.n;
  }
}

JPEG_HD int bits_get(Bits& b, int k) {      // 1 <= k <= 16
  if (b.n <= 32) bits_fill(b);
  const int v = (int)((uint32_t)(b.acc >> (b.n - k)) & ((1u << k) - 1u));
  bits_skip(b, k);
  return v;
}

JPEG_HD int huff_decode(Bits& b, const Lut& t) {      // the symbol, or -1 with err set
  const int32_t p = (int32_t)bits_peek16(b);
  int l = 1;
  JPEG_UNROLL
  for (int i = 1; i <= 16; ++i) l += p >= t.limit[i];
  if (l > 16) {
    b.err |= HRP_JPEG_ERR_CODE;
    return -1;
  }
  bits_skip(b, l);
  return t.values[((p >> (16 - l)) + t.offset[l]) & 255];
}

JPEG_HD int huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block: DC difference and AC runs into coef[64] (natural order; the caller zeroed it).  false: b.err says why.
JPEG_HD bool jpeg_decode_block(Bits& b, const Lut& dc, const Lut& ac, const uint8_t* natural, int& pred, int16_t* coef) {
  int s = huff_decode(b, dc);
  if (s < 0) return false;
  if (s > 15) {
    b.err |= HRP_JPEG_ERR_CODE;
    return false;
  }
  if (s) pred = (int16_t)(pred + huff_extend(bits_get(b, s), s));
  if (b.err) return false;
  coef[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = huff_decode(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;      // end of block
      k += 16;                 // sixteen zeros; a coefficient has to follow
      if (k > 63) {
        b.err |= HRP_JPEG_ERR_INDEX;
        return false;
      }
      continue;
    }
    k += r;
    if (k > 63) {
      b.err |= HRP_JPEG_ERR_INDEX;
      return false;
    }
    const int v = huff_extend(bits_get(b, s), s);
    if (b.err) return false;
    coef[natural[k]] = (int16_t)v;
    ++k;
  }
  return b.err == 0;
}

// One entropy-coded segment: its MCUs from s.mcu0 on, a restart interval's worth or the whole scan.  `coef` is the image's
// (zeroed) coefficient area.  Returns the HRP_JPEG_ERR_* bits.
JPEG_HD int jpeg_decode_segment(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes,
                                const Tables& t, int16_t* coef) {
  Bits b;
  bits_open(b, bytes + s.off, (size_t)s.len);
  const int total = g.mcux * g.mcuy;
  const int last = d.restart_interval ? (s.mcu0 + d.restart_interval < total ? s.mcu0 + d.restart_interval : total) : total;
  int pred[3] = {0, 0, 0};
  for (int m = s.mcu0; m < last; ++m) {
    const int my = m / g.mcux, mx = m - my * g.mcux;
    for (int c = 0; c < 3; ++c) {
      const int hs = c ? 1 : d.hsamp, vs = c ? 1 : d.vsamp;
      const Lut& dc = t.lut[d.comp_td[c]];
      const Lut& ac = t.lut[2 + d.comp_ta[c]];
      for (int v = 0; v < vs; ++v)
        for (int h = 0; h < hs; ++h) {
          const int blk = g.base[c] + (my * vs + v) * g.bw[c] + mx * hs + h;
          if (!jpeg_decode_block(b, dc, ac, t.natural, pred[c], coef + (size_t)blk * 64)) return b.err;
        }
    }
  }
  // what is left of a well-formed segment: fewer than 8 bits, all ones, and no byte
  if (b.n <= 32) bits_fill(b);
  const int real = b.n - b.fake;
  if (b.stop == HRP_JPEG_ERR_MARKER) b.err |= HRP_JPEG_ERR_MARKER;
  if (!b.stop || real >= 8 || (real > 0 && ((uint32_t)(b.acc >> b.fake) & ((1u << real) - 1u)) != (1u << real) - 1u)) b.err |= HRP_JPEG_WARN_TRAILING;
  return b.err;
}

// ---- inverse DCT ---------------------------------------------------------------------------------------------------------------
// jidctint.c's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) on coef * q; its zero-AC short cuts give the same numbers as the
// full path and are left out.  uint32_t: the sums of a damaged stream wrap as libjpeg's do on two's-complement hardware.
JPEG_HD int32_t idct_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

JPEG_HD void idct_1d(const uint32_t (&in)[8], uint32_t (&out)[8], uint32_t scale_shift) {
  const uint32_t z1e = (in[2] + in[6]) * 4433u;
  const uint32_t e2 = z1e - in[6] * 15137u, e3 = z1e + in[2] * 6270u;
  const uint32_t e0 = (in[0] + in[4]) << scale_shift, e1 = (in[0] - in[4]) << scale_shift;
  const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  uint32_t o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  uint32_t z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  o0 *= 2446u;
  o1 *= 16819u;
  o2 *= 25172u;
  o3 *= 12299u;
  z1 *= (uint32_t)-7373;
  z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  out[0] = t10 + o3;
  out[7] = t10 - o3;
  out[1] = t11 + o2;
  out[6] = t11 - o2;
  out[2] = t12 + o1;
  out[5] = t12 - o1;
  out[3] = t13 + o0;
  out[4] = t13 - o0;
}

JPEG_HD uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// coef[64] (natural order) x q[64] -> 8 x 8 samples at out, rows `stride` apart
JPEG_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, int stride) {
  uint32_t ws[8][8];      // [column][row] after pass 1
  JPEG_UNROLL
  for (int x = 0; x < 8; ++x) {
    uint32_t in[8], o[8];
    JPEG_UNROLL
    for (int y = 0; y < 8; ++y) in[y] = (uint32_t)((int32_t)coef[y * 8 + x] * (int32_t)q[y * 8 + x]);
    idct_1d(in, o, 13);
    JPEG_UNROLL
    for (int y = 0; y < 8; ++y) ws[x][y] = (uint32_t)idct_descale(o[y], 11);
  }
  JPEG_UNROLL
  for (int y = 0; y < 8; ++y) {
    uint32_t in[8], o[8];
    JPEG_UNROLL
    for (int x = 0; x < 8; ++x) in[x] = ws[x][y];
    idct_1d(in, o, 13);
    JPEG_UNROLL
    for (int x = 0; x < 8; ++x) out[(size_t)y * stride + x] = clamp_u8(idct_descale(o[x], 18) + 128);
  }
}

// block j of the image (0 <= j < g.blocks): its coefficients -> its 8 x 8 samples in the image's planes
JPEG_HD void jpeg_idct_image_block(const hrp_jpeg_image& d, const Geom& g, int j, const int16_t* coef, uint8_t* planes) {
  const int c = j >= g.base[2] ? 2 : (j >= g.base[1] ? 1 : 0);
  const int r = j - g.base[c], by = r / g.bw[c], bx = r - by * g.bw[c];
  const int stride = g.bw[c] * 8;
  jpeg_idct_block(coef + (size_t)j * 64, d.quant[d.comp_tq[c]], planes + (size_t)g.base[c] * 64 + (size_t)by * 8 * stride + bx * 8, stride);
}

// ---- up-sampling and colour ----------------------------------------------------------------------------------------------------
// jdsample.c's h2v1 / h2v2 "fancy" (triangle) up-sampling of one chroma plane at output pixel (x, y).  cw x ch real samples;
// at the edges libjpeg sees the nearest real column / row.
JPEG_HD int jpeg_chroma(const uint8_t* c, int stride, int cw, int ch, int hsamp, int vsamp, int x, int y) {
  if (hsamp == 1) return c[(size_t)y * stride + x];
  const int xi = x >> 1;
  if (vsamp == 1) {
    const uint8_t* row = c + (size_t)y * stride;
    if (x & 1) return xi == cw - 1 ? row[xi] : (3 * row[xi] + row[xi + 1] + 2) >> 2;
    return xi == 0 ? row[0] : (3 * row[xi] + row[xi - 1] + 1) >> 2;
  }
  const int r = y >> 1;
  const int f = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
  const uint8_t* near = c + (size_t)r * stride;
  const uint8_t* far = c + (size_t)f * stride;
  const int cs = 3 * near[xi] + far[xi];
  if (x & 1) {
    if (xi == cw - 1) return (4 * cs + 7) >> 4;
    return (3 * cs + 3 * near[xi + 1] + far[xi + 1] + 7) >> 4;
  }
  if (xi == 0) return (4 * cs + 8) >> 4;
  return (3 * cs + 3 * near[xi - 1] + far[xi - 1] + 8) >> 4;
}

// pixel (x, y) of the image from its planes: rgb[3], jdcolor.c's 16-bit fixed point
JPEG_HD void jpeg_pixel(const hrp_jpeg_image& d, const Geom& g, const uint8_t* planes, int x, int y, uint8_t* rgb) {
  const int yy = planes[(size_t)y * (g.bw[0] * 8) + x];
  const int cs = g.bw[1] * 8;
  const int cb = jpeg_chroma(planes + (size_t)g.base[1] * 64, cs, g.cw, g.ch, d.hsamp, d.vsamp, x, y) - 128;
  const int cr = jpeg_chroma(planes + (size_t)g.base[2] * 64, cs, g.cw, g.ch, d.hsamp, d.vsamp, x, y) - 128;
  rgb[0] = clamp_u8(yy + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp_u8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = clamp_u8(yy + ((116130 * cb + 32768) >> 16));
}

// ---- one segment decoded by many lanes (hrp_jpeg_decode_sync) --------------------------------------------------------------------
// The segment is cut into sub-sequences of S raw bytes; sub-sequence i owns every symbol (a Huffman code and its magnitude
// bits) that BEGINS in it, the last one everything to the end of the segment.  The state between two symbols is one word:
//   bits 16..  the raw bit position within the segment, 8 * byte + bit, the byte never the 00 of a stuffed FF 00; with bit 0
//              it names the next data byte (after an FF, the byte behind its 00), and at the end of the stream the byte where
//              the reader stops.  Two lanes that started at different places and fell into step give the same number.
//   bits 8..15 unit: the block's index inside the MCU, 0 .. hsamp * vsamp + 1
//   bits 0..7  k: the zig-zag index of the next coefficient, 0: a DC code comes next
// jpeg_sync_subseq decodes one sub-sequence from an entry state.  Without `fin` it writes nothing and its results are a pure
// function of the entry state and the bytes; what ends a segment in jpeg_decode_segment is met by a fixed rule instead
// (SyncSums::hit counts those events):
//   a code that does not exist,
//   a DC category above 15          16 bits are skipped and the block is abandoned: unit + 1, k = 0, not counted
//   a run past coefficient 63       the block is abandoned
//   a bit past the end of the data  the exit state is the end of the segment (bit 8 * len, unit 0, k 0), on which every later
//                                   sub-sequence decodes nothing
// Up to the first such event the chain of exit states from the true start (bit 0, unit 0, k 0) is the serial decoder's; the
// sub-sequences behind the first one with a hit are dead in the final pass.  With `fin` the entry state is the true one,
// blk0 the number of blocks the segment completed before it and pred0[] the DC predictors there (the sums of the DC
// differences so far, modulo 2^16): it writes what jpeg_decode_segment writes, stops where that stops and returns its bits.
typedef uint64_t SyncState;
constexpr SyncState SYNC_DEAD = ~(SyncState)0;
constexpr int SYNC_SERIAL = 1 << 30;      // fin: whether the status has HRP_JPEG_ERR_MARKER is for jpeg_segment_status to say

struct SyncSums {      // of the symbols that begin in one sub-sequence; after the prefix sum, of all sub-sequences before it
  uint32_t blocks;     // blocks completed
  uint16_t dc[3];      // sum of the DC differences per component, modulo 2^16
  uint16_t hit;        // events of the list above
};

JPEG_HD SyncState sync_state(uint64_t bit, int unit, int k) { return (bit << 16) | ((uint64_t)(unit & 255) << 8) | (uint64_t)(k & 255); }

// the first bit of sub-sequence i > 0 with a guessed unit and k: where every lane but the first starts
JPEG_HD SyncState sync_guess(const hrp_jpeg_image& d, const uint8_t* seg, int64_t lo, int unit, int k) {
  const int nu = d.hsamp * d.vsamp + 2;
  if (seg[lo - 1] == 0xFF && seg[lo] == 0) ++lo;      // the 00 of a stuffed pair is not data
  return sync_state((uint64_t)lo * 8, unit < 0 ? 0 : (unit < nu ? unit : nu - 1), k < 0 ? 0 : (k < 63 ? k : 63));
}

// the raw bit position of the next unread bit.  The reader has loaded up to b.p; of its look-ahead, every FF took two raw bytes.
JPEG_HD uint64_t sync_pos(const Bits& b, const uint8_t* seg) {
  const int real = b.n - b.fake, m = (real + 7) >> 3;
  int ff = 0;
  if (m) {
    uint64_t w = b.acc >> b.fake;
    if (m < 8) w &= (1ull << (8 * m)) - 1;
    w &= w >> 1;
    w &= w >> 2;
    w &= w >> 4;
    ff = __builtin_popcountll(w & 0x0101010101010101ull);
  }
  return (uint64_t)((b.p - seg) - m - ff) * 8 + (uint64_t)((8 - (real & 7)) & 7);
}

// the last MCU of a segment and the number of its blocks
JPEG_HD uint32_t sync_segment_blocks(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s) {
  const int total = g.mcux * g.mcuy;
  const int last = d.restart_interval ? (s.mcu0 + d.restart_interval < total ? s.mcu0 + d.restart_interval : total) : total;
  return (uint32_t)(last - s.mcu0) * (uint32_t)(d.hsamp * d.vsamp + 2);
}

// block `blk` of the segment in scan order, `unit` inside its MCU: its index among the image's blocks
JPEG_HD size_t sync_block(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, uint32_t blk, int unit) {
  const int nl = d.hsamp * d.vsamp, c = unit < nl ? 0 : unit - nl + 1;
  const int m = s.mcu0 + (int)(blk / (uint32_t)(nl + 2)), my = m / g.mcux, mx = m - my * g.mcux;
  const int v = c ? 0 : unit / d.hsamp, h = c ? 0 : unit - v * d.hsamp;
  return (size_t)g.base[c] + (size_t)(my * (c ? 1 : d.vsamp) + v) * g.bw[c] + mx * (c ? 1 : d.hsamp) + h;
}

// hi: the end of the sub-sequence within the segment, INT64_MAX for the last one
JPEG_HD int jpeg_sync_subseq(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes, const Tables& t,
                             int64_t hi, SyncState entry, SyncState& exit_out, SyncSums& sums_out, bool fin, uint32_t blk0, const uint16_t* pred0,
                             int16_t* coef) {
  SyncState exit = entry;      // results in registers; stored once, where the function returns
  SyncSums sums = {0, {0, 0, 0}, 0};
  auto finish = [&](int err) {
    exit_out = exit;
    sums_out = sums;
    return err;
  };
  const int nl = d.hsamp * d.vsamp, nu = nl + 2;
  int unit = (int)((entry >> 8) & 255), k = (int)(entry & 255);
  const uint64_t bit0 = entry >> 16;
  if (entry == SYNC_DEAD || unit >= nu || k > 63 || bit0 > (uint64_t)s.len * 8) {
    exit = SYNC_DEAD;
    return finish(0);
  }
  const int64_t e = (int64_t)(bit0 >> 3);
  if (e >= hi) return finish(0);      // the symbol before ran past this sub-sequence, or the stream has ended
  const uint32_t nblk = sync_segment_blocks(d, g, s);
  uint32_t blk = blk0;
  if (fin && blk >= nblk) return finish(0);      // behind the last MCU
  int16_t* out = fin ? coef + sync_block(d, g, s, blk, unit) * 64 : coef;
  const uint8_t* seg = bytes + s.off;
  Bits b;
  bits_open(b, seg + e, (size_t)(s.len - e));
  bool ended = false;      // a bit was taken that the stream does not have, at a place where jpeg_decode_block looks
  if (bit0 & 7) {
    bits_fill(b);
    bits_skip(b, (int)(bit0 & 7));
    ended = b.err != 0;
  }
  while (!ended) {
    if (b.n <= 32) bits_fill(b);      // a symbol is 32 bits at the most: no fill inside one
    const uint64_t pos = sync_pos(b, seg);
    if ((int64_t)(pos >> 3) >= hi) {
      exit = sync_state(pos, unit, k);
      return finish(0);
    }
    const int c = unit < nl ? 0 : unit - nl + 1;
    bool done = false, drop = false;      // the block is complete / abandoned
    if (k == 0) {
      const int sz = huff_decode(b, t.lut[d.comp_td[c]]);
      if (sz < 0) {
        drop = true;
      } else if (sz > 15) {
        b.err |= HRP_JPEG_ERR_CODE;
        drop = true;
      } else {
        const int diff = sz ? huff_extend(bits_get(b, sz), sz) : 0;
        if (b.err) {
          ended = true;
        } else {
          const uint16_t sum = (uint16_t)((c == 0 ? sums.dc[0] : (c == 1 ? sums.dc[1] : sums.dc[2])) + diff);      // no indexed register array
          sums.dc[0] = c == 0 ? sum : sums.dc[0];
          sums.dc[1] = c == 1 ? sum : sums.dc[1];
          sums.dc[2] = c == 2 ? sum : sums.dc[2];
          k = 1;
          if (fin) out[0] = (int16_t)(uint16_t)(pred0[c] + sum);      // the predictor: every difference of the component so far
        }
      }
    } else {
      const int rs = huff_decode(b, t.lut[2 + d.comp_ta[c]]);
      if (rs < 0) {
        drop = true;
      } else if ((rs & 15) == 0) {
        if ((rs >> 4) != 15) {      // end of block
          done = b.err == 0;
          ended = !done;
        } else {                    // sixteen zeros; a coefficient has to follow
          k += 16;
          if (k > 63) {
            b.err |= HRP_JPEG_ERR_INDEX;
            drop = true;
          }
        }
      } else {
        k += rs >> 4;
        if (k > 63) {
          b.err |= HRP_JPEG_ERR_INDEX;
          drop = true;
        } else {
          const int v = huff_extend(bits_get(b, rs & 15), rs & 15);
          if (b.err) {
            ended = true;
          } else {
            if (fin) out[t.natural[k]] = (int16_t)v;
            done = ++k == 64;
          }
        }
      }
    }
    if (ended) break;
    if (drop) {
      ++sums.hit;
      if (fin) return finish(b.err);
      if (b.err & HRP_JPEG_ERR_CODE) bits_skip(b, 16);                     // set by huff_decode or for the category: both skip
      if (b.err & (HRP_JPEG_ERR_DATA | HRP_JPEG_ERR_MARKER)) break;      // that took a bit the stream does not have: it has ended
      b.err = 0;
    }
    if (done || drop) {
      k = 0;
      unit = unit + 1 == nu ? 0 : unit + 1;
    }
    if (done) {
      ++sums.blocks;
      if (++blk == nblk && fin) {
        // Behind the last MCU: what jpeg_decode_segment checks there.  With R bits of the stream left, R < 8: its reader has
        // met the end, so has this one, and both see the same bits.  R >= 8: the warning is certain; whether that reader had
        // met a marker by then depends on how far ahead it had loaded, which only its own history says.
        if (b.n <= 32) bits_fill(b);
        const int real = b.n - b.fake;
        if (real < 8) {
          int err = b.stop == HRP_JPEG_ERR_MARKER ? HRP_JPEG_ERR_MARKER : 0;
          if (real > 0 && ((uint32_t)(b.acc >> b.fake) & ((1u << real) - 1u)) != (1u << real) - 1u) err |= HRP_JPEG_WARN_TRAILING;
          return finish(err);
        }
        const uint8_t* q = b.p;
        int stop = b.stop;
        for (int r = real; !stop && r <= 64; r += 8) {
          if (q >= b.end || (*q == 0xFF && b.end - q < 2)) stop = HRP_JPEG_ERR_DATA;
          else if (*q != 0xFF) ++q;
          else if (q[1] == 0) q += 2;
          else stop = HRP_JPEG_ERR_MARKER;
        }
        return finish(HRP_JPEG_WARN_TRAILING | (stop == HRP_JPEG_ERR_MARKER ? SYNC_SERIAL : 0));
      }
      if (fin) out = coef + sync_block(d, g, s, blk, unit) * 64;
    }
  }
  ++sums.hit;
  exit = sync_state((uint64_t)s.len * 8, 0, 0);
  return finish(fin ? b.err : 0);
}

// The status that jpeg_decode_segment returns, without its writes: `block` is 64 values of the caller's to decode into.
// For the one case above that the position alone does not settle.
JPEG_HD int jpeg_segment_status(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes, const Tables& t,
                                int16_t* block) {
  Bits b;
  bits_open(b, bytes + s.off, (size_t)s.len);
  const uint32_t nblk = sync_segment_blocks(d, g, s);
  const int nl = d.hsamp * d.vsamp, nu = nl + 2;
  int pred[3] = {0, 0, 0};
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    const int unit = (int)(blk % (uint32_t)nu), c = unit < nl ? 0 : unit - nl + 1;
    if (!jpeg_decode_block(b, t.lut[d.comp_td[c]], t.lut[2 + d.comp_ta[c]], t.natural, pred[c], block)) return b.err;
  }
  if (b.n <= 32) bits_fill(b);
  const int real = b.n - b.fake;
  if (b.stop == HRP_JPEG_ERR_MARKER) b.err |= HRP_JPEG_ERR_MARKER;
  if (!b.stop || real >= 8 || (real > 0 && ((uint32_t)(b.acc >> b.fake) & ((1u << real) - 1u)) != (1u << real) - 1u)) b.err |= HRP_JPEG_WARN_TRAILING;
  return b.err;
}

// What the lanes of one segment share, 32 bytes per sub-sequence in the caller's scratch.  The segment with index j in the list
// of long segments owns the slots from sync_region(off, j, S) on: one SyncHead, then one SyncSlot per sub-sequence.  Segments in
// ascending order that do not overlap get regions that do not overlap, inside sync_slots(nbytes, nlong, S) slots.
struct SyncSlot {
  SyncState entry, exit;
  SyncSums sums;
  uint32_t redo;       // the entry changed in this round
};
struct SyncHead {
  uint32_t rounds;     // rounds of step (b), the one in which nothing changed included
  uint32_t subseqs;
  uint32_t wrong;      // sub-sequences whose first, speculative exit state was not the final one
  uint32_t pad[5];
};
static_assert(sizeof(SyncSlot) == 32 && sizeof(SyncHead) == 32, "one slot is 32 bytes");

JPEG_HD uint64_t sync_slots(uint64_t nbytes, uint64_t nlong, uint64_t S) { return nbytes / S + 2 * nlong + 1; }
JPEG_HD uint64_t sync_region(uint64_t off, uint64_t j, uint64_t S) { return off / S + 2 * j; }
JPEG_HD int64_t sync_hi(int64_t i, int64_t n, int64_t S) { return i + 1 >= n ? INT64_MAX : (i + 1) * S; }

// step (a): sub-sequence i from the true start (i = 0) or from the guess
JPEG_HD void jpeg_sync_first(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes, const Tables& t,
                             int64_t i, int64_t n, int64_t S, int guess_unit, int guess_k, SyncSlot& sl) {
  sl.entry = i ? sync_guess(d, bytes + s.off, i * S, guess_unit, guess_k) : sync_state(0, 0, 0);
  sl.redo = 0;
  jpeg_sync_subseq(d, g, s, bytes, t, sync_hi(i, n, S), sl.entry, sl.exit, sl.sums, false, 0, nullptr, nullptr);
}

// step (c), after the prefix sum has turned sl.sums into those of everything before sub-sequence i.  The HRP_JPEG_* bits; with
// SYNC_SERIAL set when they took jpeg_segment_status (`block`: 64 values to decode into).
JPEG_HD int jpeg_sync_final(const hrp_jpeg_image& d, const Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes, const Tables& t,
                            int64_t i, int64_t n, int64_t S, const SyncSlot& sl, int16_t* coef, int16_t* block) {
  if (sl.sums.hit) return 0;      // the segment ended before this sub-sequence
  SyncState x;
  SyncSums u;
  int err = jpeg_sync_subseq(d, g, s, bytes, t, sync_hi(i, n, S), sl.entry, x, u, true, sl.sums.blocks, sl.sums.dc, coef);
  if (err & SYNC_SERIAL) err |= jpeg_segment_status(d, g, s, bytes, t, block) & HRP_JPEG_ERR_MARKER;
  return err;
}

}  // namespace jpeg
