// Baseline JPEG decode of a batch (include/hrp.h hrp_jpeg_decode): the kernels around the decoder core of jpeg_core.h.
//   clear     zeroes the coefficients (the entropy kernel writes only the non-zero ones) and the status words
//   checksum  one workgroup per image: Adler-32 of the bytes the header was parsed with against the descriptor's
//   entropy   one lane per entropy-coded segment; JPEG_LANES segments share a 64-lane wave, each with its four Huffman
//             tables in its own slice of LDS
//   sync      (hrp_jpeg_decode_sync) one workgroup per long segment: its lanes decode sub-sequences of the segment from guessed
//             states, pass exit states on in rounds until none changes, and write the coefficients in a final pass
//   idct      one lane per 8 x 8 block: dequantise + inverse DCT into the component planes
//   colour    one lane per pixel: chroma up-sampling + YCbCr -> RGB into the frame
// Every kernel checks the image's descriptor against the buffer sizes first; an image that does not fit is left alone.
#include "hrp_common.h"
#include "jpeg_core.h"

namespace hrp {
namespace {

constexpr int JPEG_THREADS = 256;
constexpr int JPEG_GRID_X = 64;        // workgroups per image of the grid-stride idct / colour launches
constexpr int JPEG_LANES = 1;          // segments per wave of the entropy kernel (1 measured against 64)
constexpr int JPEG_SYNC_THREADS = 512; // lanes of the workgroup that decodes one long segment

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_clear_kernel(uint4* __restrict__ coef, size_t n16, int32_t* __restrict__ status,
                                                                  int B) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t; i < n16; i += stride) coef[i] = make_uint4(0, 0, 0, 0);
  if (t < (size_t)B) status[t] = 0;
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_checksum_kernel(const hrp_jpeg_image* __restrict__ images,
                                                                     const uint8_t* __restrict__ bytes, size_t nbytes, size_t ncoef,
                                                                     size_t nplanes, size_t nframes, int32_t* __restrict__ status) {
  __shared__ uint32_t part[2][JPEG_THREADS];
  const hrp_jpeg_image& d = images[blockIdx.x];
  jpeg::Geom g;
  if (!jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframes)) return;      // uniform over the workgroup
  const size_t n = (size_t)d.sum_len, chunk = (n + JPEG_THREADS - 1) / JPEG_THREADS;
  const size_t lo = threadIdx.x * chunk < n ? threadIdx.x * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  jpeg::jpeg_adler_part(bytes + d.scan_off, n, lo, hi, part[0][threadIdx.x], part[1][threadIdx.x]);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0, b = 0;
    for (int i = 0; i < JPEG_THREADS; ++i) {
      a += part[0][i];
      b += part[1][i];
    }
    if (jpeg::jpeg_adler_finish(n, a, b) != d.scan_sum) atomicOr(status + blockIdx.x, HRP_JPEG_ERR_CHECKSUM);
  }
}

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const hrp_jpeg_image* __restrict__ images, int B,
                                                          const hrp_jpeg_segment* __restrict__ segments, int nseg, int lanes,
                                                          const uint8_t* __restrict__ bytes, size_t nbytes, int16_t* __restrict__ coef,
                                                          size_t ncoef, size_t nplanes, size_t nframes, int32_t* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int lane = threadIdx.x;
  const int si = blockIdx.x * lanes + lane;
  if (lane >= lanes || si >= nseg) return;
  const hrp_jpeg_segment s = segments[si];
  if (s.image < 0 || s.image >= B) return;      // no image to report to
  const hrp_jpeg_image& d = images[s.image];
  jpeg::Geom g;
  jpeg::Tables& t = ((jpeg::Tables*)lds)[lane];
  const bool ok = jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframes) && jpeg::jpeg_segment_fits(s, d, g) &&
                  jpeg::jpeg_build_tables(d, t);
  const int err = ok ? jpeg::jpeg_decode_segment(d, g, s, bytes, t, coef + d.coef_off) : HRP_JPEG_ERR_DESC;
  if (err) atomicOr(status + s.image, err);
}

// One long segment per workgroup (jpeg_core.h: "one segment decoded by many lanes").  Its sub-sequences are dealt to the lanes
// round-robin, so neighbouring lanes read neighbouring bytes.  The slots live in the caller's scratch; only this workgroup
// touches its region, and workgroup barriers order its lanes: no workgroup waits for another.
__global__ void __launch_bounds__(JPEG_SYNC_THREADS) jpeg_sync_kernel(const hrp_jpeg_image* __restrict__ images, int B,
                                                                      const hrp_jpeg_segment* __restrict__ segments, int S, int guess_unit,
                                                                      int guess_k, const uint8_t* __restrict__ bytes, size_t nbytes,
                                                                      int16_t* coef, size_t ncoef, size_t nplanes, size_t nframes,
                                                                      jpeg::SyncSlot* scratch, size_t nslots, int32_t* __restrict__ status) {
  __shared__ jpeg::Tables t;
  __shared__ jpeg::SyncSums part[JPEG_SYNC_THREADS];
  __shared__ int16_t block[64];
  __shared__ uint32_t changed_round, wrong;
  __shared__ int tables_ok;
  const int tid = threadIdx.x;
  const hrp_jpeg_segment s = segments[blockIdx.x];
  if (s.image < 0 || s.image >= B) return;      // no image to report to
  const hrp_jpeg_image& d = images[s.image];
  jpeg::Geom g;
  bool ok = jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframes) && jpeg::jpeg_segment_fits(s, d, g);
  const int64_t n = ok ? (s.len + S - 1) / S : 0;
  const uint64_t base = ok ? jpeg::sync_region((uint64_t)s.off, blockIdx.x, (uint64_t)S) : 0;
  ok = ok && base + 1 + (uint64_t)n <= nslots;
  if (tid == 0) {
    tables_ok = ok && jpeg::jpeg_build_tables(d, t);
    changed_round = wrong = 0;
  }
  __syncthreads();
  if (!tables_ok) {      // uniform over the workgroup
    if (tid == 0) atomicOr(status + s.image, HRP_JPEG_ERR_DESC);
    return;
  }
  int16_t* co = coef + d.coef_off;
  if (n == 0) {          // nothing to cut: what the one-lane kernel does
    if (tid == 0) {
      const int err = jpeg::jpeg_decode_segment(d, g, s, bytes, t, co);
      if (err) atomicOr(status + s.image, err);
    }
    return;
  }
  jpeg::SyncHead* head = (jpeg::SyncHead*)(scratch + base);
  jpeg::SyncSlot* sl = scratch + base + 1;
  // (a) every sub-sequence from its guess, the first from the true start
  for (int64_t i = tid; i < n; i += JPEG_SYNC_THREADS) jpeg::jpeg_sync_first(d, g, s, bytes, t, i, n, S, guess_unit, guess_k, sl[i]);
  __syncthreads();
  // (b) rounds: take the exit state of the sub-sequence before as it stood after the last round; decode again if it is news
  uint32_t round = 0;
  for (;;) {
    ++round;
    for (int64_t i = tid; i < n; i += JPEG_SYNC_THREADS) {
      if (i == 0) continue;
      const jpeg::SyncState e = sl[i - 1].exit;
      if (e != sl[i].entry) {
        sl[i].entry = e;
        sl[i].redo |= 1;
      }
    }
    __syncthreads();
    for (int64_t i = tid; i < n; i += JPEG_SYNC_THREADS) {
      const uint32_t redo = sl[i].redo;
      if (!(redo & 1)) continue;
      const jpeg::SyncState before = sl[i].exit;
      jpeg::jpeg_sync_subseq(d, g, s, bytes, t, jpeg::sync_hi(i, n, S), sl[i].entry, sl[i].exit, sl[i].sums, false, 0, nullptr, nullptr);
      if (redo == 1 && sl[i].exit != before) atomicAdd(&wrong, 1u);
      sl[i].redo = sl[i].exit != before ? 2 : redo & 2;
      changed_round = round;
    }
    __syncthreads();
    if (changed_round != round) break;      // written before the barrier, next written behind the next one
  }
  // (c) exclusive prefix sums of the blocks, the DC differences and the hits: a run of sub-sequences per lane, the lanes' totals
  // by lane 0
  const int64_t chunk = (n + JPEG_SYNC_THREADS - 1) / JPEG_SYNC_THREADS;
  const int64_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  auto add = [](jpeg::SyncSums& a, const jpeg::SyncSums& b) {
    a.blocks += b.blocks;
    for (int c = 0; c < 3; ++c) a.dc[c] = (uint16_t)(a.dc[c] + b.dc[c]);
    a.hit = (uint16_t)(a.hit || b.hit);
  };
  jpeg::SyncSums run = {0, {0, 0, 0}, 0};
  for (int64_t i = lo; i < hi; ++i) add(run, sl[i].sums);
  part[tid] = run;
  __syncthreads();
  if (tid == 0) {
    jpeg::SyncSums acc = {0, {0, 0, 0}, 0};
    for (int j = 0; j < JPEG_SYNC_THREADS; ++j) {
      const jpeg::SyncSums own = part[j];
      part[j] = acc;
      add(acc, own);
    }
  }
  __syncthreads();
  run = part[tid];
  for (int64_t i = lo; i < hi; ++i) {
    const jpeg::SyncSums own = sl[i].sums;
    sl[i].sums = run;
    add(run, own);
  }
  __syncthreads();
  // the final pass: the coefficients and the status, as jpeg_decode_segment leaves them
  int err = 0;
  for (int64_t i = tid; i < n; i += JPEG_SYNC_THREADS) err |= jpeg::jpeg_sync_final(d, g, s, bytes, t, i, n, S, sl[i], co, block);
  err &= ~jpeg::SYNC_SERIAL;
  if (err) atomicOr(status + s.image, err);
  if (tid == 0) {
    head->rounds = round;
    head->subseqs = (uint32_t)n;
    head->wrong = wrong;      // sub-sequences whose exit state changed after step (a)
  }
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_idct_kernel(const hrp_jpeg_image* __restrict__ images, size_t nbytes,
                                                                 const int16_t* __restrict__ coef, size_t ncoef, uint8_t* __restrict__ planes,
                                                                 size_t nplanes, size_t nframes) {
  const hrp_jpeg_image& d = images[blockIdx.y];
  jpeg::Geom g;
  if (!jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframes)) return;
  for (int j = blockIdx.x * JPEG_THREADS + threadIdx.x; j < g.blocks; j += gridDim.x * JPEG_THREADS)
    jpeg::jpeg_idct_image_block(d, g, j, coef + d.coef_off, planes + d.plane_off);
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_colour_kernel(const hrp_jpeg_image* __restrict__ images, size_t nbytes, size_t ncoef,
                                                                   const uint8_t* __restrict__ planes, size_t nplanes, uint8_t* __restrict__ frames,
                                                                   size_t nframes) {
  const hrp_jpeg_image& d = images[blockIdx.y];
  jpeg::Geom g;
  if (!jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframes)) return;
  const int n = d.width * d.height;
  uint8_t* out = frames + d.frame_off;
  for (int i = blockIdx.x * JPEG_THREADS + threadIdx.x; i < n; i += gridDim.x * JPEG_THREADS) {
    const int y = i / d.width, x = i - y * d.width;
    uint8_t rgb[3];
    jpeg::jpeg_pixel(d, g, planes + d.plane_off, x, y, rgb);
    out[(size_t)i * 3 + 0] = rgb[0];
    out[(size_t)i * 3 + 1] = rgb[1];
    out[(size_t)i * 3 + 2] = rgb[2];
  }
}

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_jpeg_decode_stage(int stage, int lanes, const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* segments_dev,
                                     int nseg, const uint8_t* bytes, size_t nbytes, int16_t* coef, size_t ncoef, uint8_t* planes,
                                     size_t nplanes, uint8_t* frames, size_t nframes, int32_t* status, void* stream) {
  HRP_REQUIRE(images_dev && segments_dev && bytes && coef && planes && frames && status, "jpeg_decode: null buffer");
  HRP_REQUIRE(B > 0 && B <= 65535 && nseg > 0, "jpeg_decode: %d images, %d segments", B, nseg);
  HRP_REQUIRE(((uintptr_t)coef & 15) == 0 && ncoef % 64 == 0, "jpeg_decode: coef must be 16-byte aligned, a multiple of 64 values");
  HRP_REQUIRE(stage == 0 || stage == 1, "jpeg_decode: stage %d", stage);
  if (lanes == 0) lanes = JPEG_LANES;
  HRP_REQUIRE(lanes >= 1 && lanes <= 64, "jpeg_decode: %d segments per wave", lanes);
  hipStream_t s = (hipStream_t)stream;
  if (stage == 0) {
    const size_t n16 = ncoef / 8;
    size_t blocks = (n16 + JPEG_THREADS - 1) / JPEG_THREADS;
    const size_t need = ((size_t)B + JPEG_THREADS - 1) / JPEG_THREADS;
    blocks = blocks > 2048 ? 2048 : blocks;
    blocks = blocks < need ? need : blocks;
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)blocks), dim3(JPEG_THREADS), 0, s, (uint4*)coef, n16, status, B);
    hipLaunchKernelGGL(jpeg_checksum_kernel, dim3(B), dim3(JPEG_THREADS), 0, s, images_dev, bytes, nbytes, ncoef, nplanes, nframes, status);
    const size_t lds = (size_t)lanes * sizeof(jpeg::Tables);
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute((const void*)jpeg_entropy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      attr = true;
    }
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)cdiv(nseg, lanes)), dim3(64), lds, s, images_dev, B, segments_dev, nseg, lanes,
                       bytes, nbytes, coef, ncoef, nplanes, nframes, status);
    return check_launch("jpeg_decode (entropy)");
  }
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(JPEG_GRID_X, B), dim3(JPEG_THREADS), 0, s, images_dev, nbytes, coef, ncoef, planes, nplanes,
                     nframes);
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(JPEG_GRID_X, B), dim3(JPEG_THREADS), 0, s, images_dev, nbytes, ncoef, planes, nplanes,
                     frames, nframes);
  return check_launch("jpeg_decode (pixels)");
}

extern "C" int hrp_jpeg_decode(const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* segments_dev, int nseg, const uint8_t* bytes,
                               size_t nbytes, int16_t* coef, size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frames, size_t nframes,
                               int32_t* status, void* stream) {
  const int rc = hrp_jpeg_decode_stage(0, 0, images_dev, B, segments_dev, nseg, bytes, nbytes, coef, ncoef, planes, nplanes, frames,
                                       nframes, status, stream);
  if (rc) return rc;
  return hrp_jpeg_decode_stage(1, 0, images_dev, B, segments_dev, nseg, bytes, nbytes, coef, ncoef, planes, nplanes, frames, nframes,
                               status, stream);
}

extern "C" size_t hrp_jpeg_sync_scratch_bytes(size_t nbytes, int nlong, int subseq_bytes) {
  if (nlong < 0 || subseq_bytes < 16 || subseq_bytes > 4096 || (subseq_bytes & (subseq_bytes - 1))) return 0;
  return (size_t)jpeg::sync_slots(nbytes, (uint64_t)nlong, (uint64_t)subseq_bytes) * sizeof(jpeg::SyncSlot);
}

extern "C" int hrp_jpeg_decode_sync_stage(int stage, int guess_unit, int guess_k, const hrp_jpeg_image* images_dev, int B,
                                          const hrp_jpeg_segment* short_segments_dev, int nshort, const hrp_jpeg_segment* long_segments_dev,
                                          int nlong, int subseq_bytes, const uint8_t* bytes, size_t nbytes, int16_t* coef, size_t ncoef,
                                          uint8_t* planes, size_t nplanes, uint8_t* frames, size_t nframes, void* scratch, size_t nscratch,
                                          int32_t* status, void* stream) {
  HRP_REQUIRE(images_dev && bytes && coef && planes && frames && status && scratch, "jpeg_decode_sync: null buffer");
  HRP_REQUIRE(B > 0 && B <= 65535 && nshort >= 0 && nlong >= 0 && nshort + (int64_t)nlong > 0, "jpeg_decode_sync: %d images, %d + %d segments", B,
              nshort, nlong);
  HRP_REQUIRE((nshort == 0 || short_segments_dev) && (nlong == 0 || long_segments_dev), "jpeg_decode_sync: null segment list");
  HRP_REQUIRE(((uintptr_t)coef & 15) == 0 && ncoef % 64 == 0, "jpeg_decode_sync: coef must be 16-byte aligned, a multiple of 64 values");
  HRP_REQUIRE(subseq_bytes >= 16 && subseq_bytes <= 4096 && !(subseq_bytes & (subseq_bytes - 1)),
              "jpeg_decode_sync: sub-sequences of %d bytes, want a power of two in 16 .. 4096", subseq_bytes);
  HRP_REQUIRE(((uintptr_t)scratch & 15) == 0 && nscratch >= hrp_jpeg_sync_scratch_bytes(nbytes, nlong, subseq_bytes),
              "jpeg_decode_sync: scratch must be 16-byte aligned and hold hrp_jpeg_sync_scratch_bytes() = %zu bytes, got %zu",
              hrp_jpeg_sync_scratch_bytes(nbytes, nlong, subseq_bytes), nscratch);
  HRP_REQUIRE(stage == 0 || stage == 1, "jpeg_decode_sync: stage %d", stage);
  hipStream_t s = (hipStream_t)stream;
  if (stage == 1)
    return hrp_jpeg_decode_stage(1, 0, images_dev, B, nshort ? short_segments_dev : long_segments_dev, nshort ? nshort : nlong, bytes, nbytes,
                                 coef, ncoef, planes, nplanes, frames, nframes, status, stream);
  const size_t n16 = ncoef / 8;
  size_t blocks = (n16 + JPEG_THREADS - 1) / JPEG_THREADS;
  const size_t need = ((size_t)B + JPEG_THREADS - 1) / JPEG_THREADS;
  blocks = blocks > 2048 ? 2048 : blocks;
  blocks = blocks < need ? need : blocks;
  hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)blocks), dim3(JPEG_THREADS), 0, s, (uint4*)coef, n16, status, B);
  hipLaunchKernelGGL(jpeg_checksum_kernel, dim3(B), dim3(JPEG_THREADS), 0, s, images_dev, bytes, nbytes, ncoef, nplanes, nframes, status);
  if (nshort)
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)cdiv(nshort, JPEG_LANES)), dim3(64), JPEG_LANES * sizeof(jpeg::Tables), s, images_dev, B,
                       short_segments_dev, nshort, JPEG_LANES, bytes, nbytes, coef, ncoef, nplanes, nframes, status);
  if (nlong)
    hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)nlong), dim3(JPEG_SYNC_THREADS), 0, s, images_dev, B, long_segments_dev, subseq_bytes,
                       guess_unit, guess_k, bytes, nbytes, coef, ncoef, nplanes, nframes, (jpeg::SyncSlot*)scratch,
                       nscratch / sizeof(jpeg::SyncSlot), status);
  return check_launch("jpeg_decode_sync (entropy)");
}

extern "C" int hrp_jpeg_decode_sync(const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* short_segments_dev, int nshort,
                                    const hrp_jpeg_segment* long_segments_dev, int nlong, int subseq_bytes, const uint8_t* bytes, size_t nbytes,
                                    int16_t* coef, size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frames, size_t nframes, void* scratch,
                                    size_t nscratch, int32_t* status, void* stream) {
  const int rc = hrp_jpeg_decode_sync_stage(0, 0, 0, images_dev, B, short_segments_dev, nshort, long_segments_dev, nlong, subseq_bytes, bytes,
                                            nbytes, coef, ncoef, planes, nplanes, frames, nframes, scratch, nscratch, status, stream);
  if (rc) return rc;
  return hrp_jpeg_decode_sync_stage(1, 0, 0, images_dev, B, short_segments_dev, nshort, long_segments_dev, nlong, subseq_bytes, bytes, nbytes,
                                    coef, ncoef, planes, nplanes, frames, nframes, scratch, nscratch, status, stream);
}
