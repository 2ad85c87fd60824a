"""Host side of the device JPEG decode (csrc/jpeg.hip, include/hrp.h hrp_jpeg_decode).

``parse_header`` reads a file's markers up to SOS into one hrp_jpeg_image record (as a fixed-size uint8 array, which the default
collate stacks), or returns None for a file the device path does not take: progressive or arithmetic coding, 12 bit, one or four
components, sampling other than 4:4:4 / 4:2:2 / 4:2:0, several scans, an Adobe marker announcing another colour transform, or a
down-sampled chroma plane of two columns or fewer.  ``decode_batch`` uploads the files' bytes in one copy, splits every scan at
its restart markers, fills in the offsets and launches the decode; the frames equal Pillow's (libjpeg-turbo defaults) byte for
byte.  ``status`` stays on the device: ``check_status`` is the call that synchronises and raises.  There is no CPU path.

``entropy="sync"`` (``Batch``, ``decode_batch``; default ``"segment"``) selects hrp_jpeg_decode_sync: segments of at least
``min_subseq`` sub-sequences of ``subseq_bytes`` bytes - a file without restart markers is one such segment - are decoded by one
workgroup each from speculative start points, the others by the one-lane kernel as before.  Same frames, coefficients and status.
"""
import zlib

import numpy as np
import torch

from hrpe_amd import _native as nv

HDR_DTYPE = np.dtype(nv.JpegImage)
SEG_DTYPE = np.dtype(nv.JpegSegment)
HDR_BYTES = HDR_DTYPE.itemsize
# entropy="sync": the sub-sequence size (the fastest of 32 / 64 / 128 / 256 on 127 KB scans), and how many sub-sequences make a
# segment a long one (the smallest value that keeps 4.2 KB restart intervals on the one-lane kernel, where they are faster).
# DESIGN 7.7 has the measurements.
SUBSEQ_BYTES = 256
MIN_SUBSEQ = 18
ERR_MASK = nv.JPEG_ERR_DATA | nv.JPEG_ERR_MARKER | nv.JPEG_ERR_CODE | nv.JPEG_ERR_INDEX | nv.JPEG_ERR_DESC | nv.JPEG_ERR_CHECKSUM

# zig-zag position -> natural (row-major) index
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                    61, 54, 47, 55, 62, 63])


def record(hdr):
    """The hrp_jpeg_image view (numpy structured scalar or array) of what parse_header returned, or of a collated stack."""
    if isinstance(hdr, (np.ndarray, np.void)) and hdr.dtype == HDR_DTYPE:
        return hdr
    a = np.ascontiguousarray(np.asarray(hdr, dtype=np.uint8))
    if a.shape[-1] != HDR_BYTES:
        raise nv.HrpError(f"jpeg header record of {a.shape[-1]} bytes, want {HDR_BYTES}")
    v = a.view(HDR_DTYPE)
    return v.reshape(a.shape[:-1]) if a.ndim > 1 else v[0]


def blocks_of(width, height, hsamp, vsamp):
    """8 x 8 blocks of the image's three component planes, whole MCUs."""
    mcux, mcuy = -(-int(width) // (8 * int(hsamp))), -(-int(height) // (8 * int(vsamp)))
    return mcux * mcuy * (int(hsamp) * int(vsamp) + 2)


def parse_header(data):
    """One pass over the markers of `data` (bytes) up to SOS.  Returns a uint8 [HDR_BYTES] array holding an hrp_jpeg_image
    (scan_off: the first entropy-coded byte within the file, scan_len: from there to the end of the file; the buffer offsets
    zero), or None when the file is not for the device path.  Every length is checked against the file."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    rec = np.zeros(1, dtype=HDR_DTYPE)
    r = rec[0]
    have_q, have_h = set(), set()
    comps = None
    pos = 2
    while True:
        if pos + 4 > n or data[pos] != 0xFF:
            return None
        m = data[pos + 1]
        if m == 0xFF:                       # fill byte
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD9:  # no segment here before SOS in a file we take
            return None
        ln = (data[pos + 2] << 8) | data[pos + 3]
        if ln < 2 or pos + 2 + ln > n:
            return None
        seg = data[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xDB:                       # DQT
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0 or tq > 3 or i + 65 > len(seg):
                    return None
                r["quant"][tq][NATURAL] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=i + 1)
                have_q.add(tq)
                i += 65
        elif m == 0xC4:                     # DHT
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                if tc > 1 or th > 1 or i + 17 > len(seg):
                    return None
                counts = np.frombuffer(seg, dtype=np.uint8, count=16, offset=i + 1)
                nv_ = int(counts.sum())
                if nv_ > 256 or i + 17 + nv_ > len(seg):
                    return None
                code = 0
                for length, c in enumerate(counts, 1):     # the codes must fit their lengths
                    code += int(c)
                    if code > (1 << length):
                        return None
                    code <<= 1
                t = r["ac" if tc else "dc"][th]
                t["counts"] = counts
                t["values"] = 0
                t["values"][:nv_] = np.frombuffer(seg, dtype=np.uint8, count=nv_, offset=i + 17)
                have_h.add((tc, th))
                i += 17 + nv_
        elif m == 0xC0:                     # SOF0
            if comps is not None or len(seg) < 6:
                return None
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8 or nc != 3 or h < 1 or w < 1 or len(seg) != 6 + 3 * nc:
                return None
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
            if tuple(c[0] for c in comps) == (82, 71, 66):      # components named R, G, B: libjpeg does not convert them
                return None
            r["width"], r["height"] = w, h
        elif m == 0xDD:                     # DRI
            if len(seg) != 2:
                return None
            r["restart_interval"] = (seg[0] << 8) | seg[1]
        elif m == 0xEE:                     # Adobe: transform 1 is YCbCr
            if len(seg) >= 12 and seg[:5] == b"Adobe" and seg[11] != 1:
                return None
        elif m == 0xDA:                     # SOS
            if comps is None or len(seg) != 4 + 2 * 3 or seg[0] != 3:
                return None
            for c in range(3):
                if seg[1 + 2 * c] != comps[c][0]:
                    return None
                td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if td > 1 or ta > 1 or (0, td) not in have_h or (1, ta) not in have_h or comps[c][3] not in have_q:
                    return None
                r["comp_td"][c], r["comp_ta"][c], r["comp_tq"][c] = td, ta, comps[c][3]
            if (seg[7], seg[8], seg[9]) != (0, 63, 0):
                return None
            break
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass                            # APPn, COM
        else:
            return None                     # SOF1..15 (extended, progressive, lossless, arithmetic), DAC, DNL, ...
    (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = comps
    if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
        return None
    w = int(r["width"])
    if h0 == 2 and -(-w // 2) <= 2:         # libjpeg replicates instead of filtering a chroma row this short
        return None
    r["hsamp"], r["vsamp"] = h0, v0
    r["scan_off"], r["scan_len"], r["sum_len"] = pos, n - pos, n - pos
    r["scan_sum"] = zlib.adler32(memoryview(data)[pos:])
    return rec.view(np.uint8).reshape(HDR_BYTES).copy()


def split_segments(buf, recs):
    """buf: the concatenated files (uint8 array); recs: hrp_jpeg_image records whose scan_off / scan_len are already offsets
    into buf, scan_len reaching the end of the image's file.  Finds every marker of every scan in one vectorised pass, cuts
    scan_len at the first marker that is not RSTn and returns the hrp_jpeg_segment records.  A scan whose restart markers do
    not match its restart interval raises."""
    ff = np.flatnonzero(buf[:-1] == 0xFF)
    nxt = buf[ff + 1]
    keep = nxt != 0
    mpos, mval = ff[keep], nxt[keep]
    segs = []
    for i, r in enumerate(recs):
        a, e = int(r["scan_off"]), int(r["scan_off"]) + int(r["scan_len"])
        lo, hi = np.searchsorted(mpos, a), np.searchsorted(mpos, e - 1)
        p, v = mpos[lo:hi], mval[lo:hi]
        stop = np.flatnonzero((v < 0xD0) | (v > 0xD7))
        k = int(stop[0]) if len(stop) else len(p)
        end = int(p[k]) if len(stop) else e
        total = -(-int(r["width"]) // (8 * int(r["hsamp"]))) * -(-int(r["height"]) // (8 * int(r["vsamp"])))
        ri = int(r["restart_interval"])
        want = -(-total // ri) if ri else 1
        if len(stop) and v[k] != 0xD9:
            raise nv.HrpError(f"jpeg image {i}: marker FF{int(v[k]):02X} after the scan (several scans are not decoded on the device)")
        if k + 1 != want:
            raise nv.HrpError(f"jpeg image {i}: {k} restart markers in the scan, restart interval {ri} over {total} MCUs needs {want - 1}")
        if ((v[:k] - 0xD0) != (np.arange(k) & 7)).any():
            raise nv.HrpError(f"jpeg image {i}: restart markers out of order")
        s = np.zeros(k + 1, dtype=SEG_DTYPE)
        s["off"] = np.concatenate([[a], p[:k] + 2])
        s["len"] = np.concatenate([p[:k], [end]]) - s["off"]
        s["image"] = i
        s["mcu0"] = np.arange(k + 1) * ri
        r["scan_len"] = end - a
        segs.append(s)
    return np.concatenate(segs)


def split_long(segs, subseq_bytes, min_subseq):
    """(short, long): the segments that span fewer than min_subseq sub-sequences of subseq_bytes bytes, and the others; both in
    the order of `segs` (ascending offsets, as hrp_jpeg_decode_sync wants its long list)."""
    is_long = -(-segs["len"].astype(np.int64) // int(subseq_bytes)) >= int(min_subseq)
    is_long &= segs["len"] > 0
    return segs[~is_long], segs[is_long]


class Batch:
    """The buffers of one decode on the device, and the arguments of hrp_jpeg_decode for them (a fixed set of caller-owned
    buffers: ``launch`` can be captured in a graph and replayed).  entropy="sync": of hrp_jpeg_decode_sync, with ``scratch``
    among the buffers and the segments in two lists, ``short`` and ``long``."""

    def __init__(self, datas, records, device, entropy="segment", subseq_bytes=None, min_subseq=None):
        if entropy not in ("segment", "sync"):
            raise nv.HrpError(f"jpeg Batch: entropy {entropy!r}, want 'segment' or 'sync'")
        S = SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
        m = MIN_SUBSEQ if min_subseq is None else int(min_subseq)
        if entropy == "sync" and (S < 16 or S > 4096 or S & (S - 1) or m < 1):
            raise nv.HrpError(f"jpeg Batch: sub-sequences of {S} bytes (want a power of two in 16 .. 4096), min_subseq {m} (want >= 1)")
        if entropy == "sync" and torch.device(device).type != "cuda":
            raise nv.HrpError(f"jpeg Batch: {device} is not a GPU (there is no CPU path)")
        self.entropy, self.subseq_bytes, self.min_subseq = entropy, S, m
        recs = np.array(record(records), dtype=HDR_DTYPE, ndmin=1).copy()
        B = len(datas)
        if B < 1 or recs.shape != (B,):
            raise nv.HrpError(f"jpeg decode_batch: {B} files, {recs.shape} header records")
        sizes = np.array([len(d) for d in datas], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        if ((recs["scan_off"] < 0) | (recs["scan_off"] > sizes) | (recs["scan_len"] != sizes - recs["scan_off"]) |
                (recs["sum_len"] != recs["scan_len"])).any():
            raise nv.HrpError("jpeg decode_batch: a header record does not belong to its file")
        if ((recs["width"] < 1) | (recs["height"] < 1) | (recs["width"] > 16384) | (recs["height"] > 16384)).any():
            raise nv.HrpError("jpeg decode_batch: image size outside 1 .. 16384")
        buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
        recs["scan_off"] += starts
        segs = split_segments(buf, recs)
        blocks = np.array([blocks_of(r["width"], r["height"], r["hsamp"], r["vsamp"]) for r in recs], dtype=np.int64)
        fbytes = recs["width"].astype(np.int64) * recs["height"] * 3
        recs["coef_off"] = np.concatenate([[0], np.cumsum(blocks * 64)[:-1]])
        recs["plane_off"] = recs["coef_off"]
        recs["frame_off"] = np.concatenate([[0], np.cumsum(fbytes)[:-1]])
        self.records, self.segments, self.B = recs, segs, B
        self.shapes = [(int(r["height"]), int(r["width"])) for r in recs]
        up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(device, non_blocking=True)   # noqa: E731
        self.images_d, self.segments_d, self.bytes_d = up(recs), up(segs), up(buf)
        if entropy == "sync":
            self.short, self.long = split_long(segs, S, m)
            self.short_d, self.long_d = (up(a) if len(a) else None for a in (self.short, self.long))
            self.scratch = torch.empty(32 * (len(buf) // S + 2 * len(self.long) + 1), dtype=torch.uint8, device=device)
        ncoef = int(blocks.sum()) * 64
        self.coef = torch.empty(ncoef, dtype=torch.int16, device=device)
        self.planes = torch.empty(ncoef, dtype=torch.uint8, device=device)
        self.flat = torch.empty(int(fbytes.sum()), dtype=torch.uint8, device=device)
        self.status = torch.empty(B, dtype=torch.int32, device=device)

    def args(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.flat.device).cuda_stream
        return (self.images_d.data_ptr(), self.B, self.segments_d.data_ptr(), len(self.segments), self.bytes_d.data_ptr(),
                self.bytes_d.numel(), self.coef.data_ptr(), self.coef.numel(), self.planes.data_ptr(), self.planes.numel(),
                self.flat.data_ptr(), self.flat.numel(), self.status.data_ptr(), s)

    def sync_args(self, stream=None):
        """The arguments of hrp_jpeg_decode_sync (entropy="sync")."""
        a = self.args(stream)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        return (a[0], a[1], ptr(self.short_d), len(self.short), ptr(self.long_d), len(self.long), self.subseq_bytes) + a[4:12] + \
            (self.scratch.data_ptr(), self.scratch.numel()) + a[12:]

    def launch(self, stream=None):
        if self.entropy == "sync":
            nv.call("hrp_jpeg_decode_sync", *self.sync_args(stream))
        else:
            nv.call("hrp_jpeg_decode", *self.args(stream))

    def rounds(self):
        """entropy="sync", after a launch (synchronises): the rounds each long segment's workgroup needed, the last one - in
        which nothing changed - included."""
        if not len(self.long):
            return np.zeros(0, dtype=np.uint32)
        slot = self.long["off"].astype(np.int64) // self.subseq_bytes + 2 * np.arange(len(self.long))
        return self.scratch.view(torch.int32)[torch.as_tensor(slot * 8, device=self.scratch.device)].cpu().numpy().astype(np.uint32)

    def frames(self):
        """One [H, W, 3] uint8 view of the frame buffer per image."""
        offs = self.records["frame_off"]
        return [self.flat[int(o):int(o) + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offs, self.shapes)]


def decode_batch(datas, records, device, stream=None, entropy="segment", subseq_bytes=None, min_subseq=None):
    """datas: list of the files' bytes; records: their parse_header results (a list, or the collated [B, HDR_BYTES] array /
    tensor).  One upload, one hrp_jpeg_decode call on `stream` (default: the current stream); entropy="sync": one
    hrp_jpeg_decode_sync call (see Batch).  Returns (frames, status): a list of uint8 [H, W, 3] device tensors (views of one
    buffer) and the int32 [B] status on the device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise nv.HrpError(f"jpeg decode_batch: {device} is not a GPU (there is no CPU path)")
    nv.lib()
    if not isinstance(records, (np.ndarray, torch.Tensor)):
        if any(r is None for r in records):
            raise nv.HrpError("jpeg decode_batch: a file without a header record (parse_header refused it: decode it on the host)")
        records = np.stack([np.asarray(r, dtype=np.uint8) for r in records])
    b = Batch(datas, records, device, entropy=entropy, subseq_bytes=subseq_bytes, min_subseq=min_subseq)
    b.launch(stream)
    return b.frames(), b.status


def check_status(status):
    """Synchronises on `status` and raises HrpError naming the images whose scan did not decode.  HRP_JPEG_WARN_TRAILING alone
    (every MCU decoded, data left over) does not raise; returns the status as a numpy array."""
    st = status.cpu().numpy()
    bad = np.flatnonzero(st & ERR_MASK)
    if len(bad):
        raise nv.HrpError("jpeg decode: " + ", ".join(f"image {i} status {int(st[i])}" for i in bad[:8]) +
                          " (1 out of data, 2 marker in a segment, 4 no such code, 8 coefficient index, 16 descriptor, "
                          "64 the bytes are not the ones the header was parsed from)")
    return st
