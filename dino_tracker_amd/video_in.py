"""JPEG ingest on the device: the files' bytes go up once, and entropy decoding, dequantisation, inverse DCT, chroma upsampling and
colour conversion run in libdtk (csrc/jpeg_decode.hip; the arithmetic is defined in docs/JPEG_DECODE.md and is bit-equal to Pillow's
decoder for the files an encoder makes).  The host only reads headers:

    parse_jpeg_sampled(data)                  (JpegHeader, None) for a file the device decodes, else (None, the reason)
    plan_jpeg_sampled(datas)                  the headers of several files of one size and sampling as the arrays the library takes
    parse_jpeg(data), plan_jpeg(datas)        the same, for 4:2:0 files without an Adobe segment only
    decode_jpeg(files_or_bytes, device)       uint8 [T, H, W, 3] on the device, [T, H, W, 1] for gray files
    decode_jpeg_coefficients(...)             the entropy stage alone: (int16 [T, MCUs, B, 64] zigzag, int32 status [T], plan)
    entropy_mode(entropy)                     "sequential" (one lane per segment) or "parallel" (a workgroup per segment: for files
                                              without restart markers), from the argument or DTK_JPEG_ENTROPY; the frames are the same

    parse_jpeg_progressive(data), scan_levels(scans), plan_jpeg_progressive(datas), decode_jpeg_progressive(...),
    decode_jpeg_progressive_coefficients(...)  the same for PROGRESSIVE files (SOF2), through their own entry points only

Decoded on the device: baseline sequential (SOF0), 8 bit, ONE scan (Ss = 0, Se = 63, Ah = Al = 0) of either components 1, 2, 3
interleaved and sampled 2x2 / 1x1 / 1x1 (4:2:0), 2x1 / 1x1 / 1x1 (4:2:2) or 1x1 / 1x1 / 1x1 (4:4:4), or of one component with id 1
(gray, whatever sampling factors its SOF names); 8-bit quantisation tables, any Huffman tables, any restart interval; an Adobe APP14
segment only on three components and only with transform 1 (YCbCr).  Progressive files (SOF2) of the same
layouts with a legal and complete scan script are decoded by the *_progressive functions (further down) and by none of the others.
Everything else -- and every file whose header this parser
cannot follow -- is reported with its reason and stays with the caller's host path."""
from __future__ import annotations

import io
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

HUFF_BYTES = 272          # DTK_JPEG_HUFF_BYTES: 16 counts + up to 256 symbols
SEGMENT_MAX_BYTES = 1 << 28
S420, S422, S444, GRAY = ops.JPEG_420, ops.JPEG_422, ops.JPEG_444, ops.JPEG_GRAY
SAMPLING_NAMES = ops.JPEG_SAMPLING_NAMES
mcus_of = ops.jpeg_mcus          # (height, width, sampling) -> MCUs of a frame
_FACTORS = {(0x22, 0x11, 0x11): S420, (0x21, 0x11, 0x11): S422, (0x11, 0x11, 0x11): S444}
_FACTOR_NAMES = {(0x22, 0x11, 0x11): "4:2:0", (0x21, 0x11, 0x11): "4:2:2", (0x11, 0x11, 0x11): "4:4:4", (0x12, 0x11, 0x11): "4:4:0",
                 (0x41, 0x11, 0x11): "4:1:1"}


@dataclass
class JpegHeader:
    height: int
    width: int
    qtables: np.ndarray          # uint8 [C, 64]: per component (C = 3, gray: 1), zigzag order (as DQT stores them)
    huffman: np.ndarray          # uint8 [C, 2, 272]: per component the DC and the AC table, counts then symbols
    restart: int                 # MCUs per restart interval, 0: none
    scan: Tuple[int, int]        # byte range of the entropy-coded data (RSTn markers included, EOI excluded)
    segments: np.ndarray         # int64 [S, 4]: byte offset in the file, byte length, first MCU, MCU count
    sampling: int = S420         # S420, S422, S444 or GRAY
    adobe: bool = False          # an Adobe APP14 segment with transform 1 stands in the file

    @property
    def mcus(self) -> int:
        return mcus_of(self.height, self.width, self.sampling)


_SOF_OTHERS = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential (SOF5)",
               0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
               0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)", 0xCD: "arithmetic coding (SOF13)",
               0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def _check_huffman(cls: int, counts: Sequence[int], vals: bytes) -> Optional[str]:
    if sum(counts) > 256 or len(vals) != sum(counts):
        return "DHT: more than 256 symbols, or the segment is short"
    code = 0
    for length, n in enumerate(counts, 1):
        code += n
        if code > (1 << length):
            return f"DHT: length {length} is over-subscribed"
        code <<= 1
    if cls == 0 and any(v > 11 for v in vals):
        return "DHT: a DC category above 11"
    if cls == 1 and any((v & 15) > 10 for v in vals):
        return "DHT: an AC size above 10"
    return None


def parse_jpeg(data) -> Tuple[Optional[JpegHeader], Optional[str]]:
    """Walk SOI .. SOS of one file (bytes, memoryview or uint8 array).  (header, None) for a 4:2:0 file without an Adobe segment
    that the device decodes, else (None, why)."""
    return _parse(data, wide=False)


def parse_jpeg_sampled(data) -> Tuple[Optional[JpegHeader], Optional[str]]:
    """parse_jpeg for every layout the device decodes (module docstring): the header names its `sampling`."""
    return _parse(data, wide=True)


def _parse(data, wide: bool) -> Tuple[Optional[JpegHeader], Optional[str]]:
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = int(buf.shape[0])
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        return None, "no SOI marker"
    dqt, dht, restart, sof, adobe = {}, {}, 0, None, None
    i = 2
    while True:
        if i + 4 > n or buf[i] != 0xFF:
            return None, f"no marker at byte {i}"
        marker = int(buf[i + 1])
        if marker == 0xFF:          # a fill byte
            i += 1
            continue
        if marker in _SOF_OTHERS:
            return None, _SOF_OTHERS[marker]
        if marker == 0x01 or 0xD0 <= marker <= 0xD9 or marker == 0x00:
            return None, f"marker FF{marker:02X} before the scan"
        length = (int(buf[i + 2]) << 8) | int(buf[i + 3])
        if length < 2 or i + 2 + length > n:
            return None, f"segment FF{marker:02X} at byte {i} runs past the file"
        seg = bytes(buf[i + 4:i + 2 + length])
        i += 2 + length
        if marker == 0xDB:
            k = 0
            while k < len(seg):
                if seg[k] >> 4:
                    return None, "16-bit quantisation table"
                if (seg[k] & 15) > 3 or k + 65 > len(seg):
                    return None, "DQT: table id above 3, or the segment is short"
                dqt[seg[k] & 15] = np.frombuffer(seg[k + 1:k + 65], dtype=np.uint8)
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg) or (seg[k] >> 4) > 1 or (seg[k] & 15) > 3:
                    return None, "DHT: table class above 1, id above 3, or the segment is short"
                counts = list(seg[k + 1:k + 17])
                vals = seg[k + 17:k + 17 + sum(counts)]
                why = _check_huffman(seg[k] >> 4, counts, vals)
                if why:
                    return None, why
                dht[seg[k]] = bytes(counts) + vals
                k += 17 + sum(counts)
        elif marker == 0xDD:
            if len(seg) != 2:
                return None, "DRI: wrong length"
            restart = (seg[0] << 8) | seg[1]
        elif marker == 0xEE:
            if seg[:5] == b"Adobe":
                adobe = seg[11] if len(seg) >= 12 else -1
        elif marker == 0xC0:
            if sof is not None:
                return None, "two SOF0 segments"
            sof = seg
        elif marker == 0xDA:
            break
    if adobe is not None and not wide:
        return None, "Adobe APP14 segment"
    if sof is None or len(sof) < 6:
        return None, "no SOF0 segment before the scan"
    if sof[0] != 8:
        return None, f"{sof[0]}-bit samples"
    height, width, ncomp = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    if ncomp not in ((1, 3) if wide else (3,)) or len(sof) != 6 + 3 * ncomp:
        return None, "grayscale (1 component)" if ncomp == 1 else f"{ncomp} components"
    if adobe is not None and (ncomp != 3 or adobe != 1):
        return None, (f"Adobe APP14 segment on {ncomp} component" if ncomp != 3 else
                      f"Adobe APP14 segment with transform {adobe}, not 1 (YCbCr)" if adobe >= 0 else "Adobe APP14 segment is short")
    if height < 1 or width < 1:
        return None, "zero height or width (DNL)"
    comps = [(sof[6 + 3 * c], sof[7 + 3 * c], sof[8 + 3 * c]) for c in range(ncomp)]
    if [c[0] for c in comps] != [1, 2, 3][:ncomp]:
        return None, f"component ids {[c[0] for c in comps]}, not {'1 2 3' if ncomp == 3 else '1'}"
    factors = tuple(c[1] for c in comps)
    if ncomp == 1:
        sampling = GRAY          # a single-component scan is not interleaved: its factors change nothing
    elif factors in _FACTORS and (wide or factors == (0x22, 0x11, 0x11)):
        sampling = _FACTORS[factors]
    else:
        return None, (f"sampling {_FACTOR_NAMES.get(factors, [hex(v) for v in factors])}, not " +
                      ("4:2:0, 4:2:2 or 4:4:4" if wide else "4:2:0"))
    if any(c[2] not in dqt for c in comps):
        return None, "a component's quantisation table is not defined"
    if len(seg) != 4 + 2 * ncomp or seg[0] != ncomp:
        return None, "several scans (the first does not hold all three components)"
    if [seg[1 + 2 * c] for c in range(ncomp)] != [1, 2, 3][:ncomp]:
        return None, "scan components out of order"
    if tuple(seg[1 + 2 * ncomp:4 + 2 * ncomp]) != (0, 63, 0):
        return None, "the scan is not Ss = 0, Se = 63, Ah = Al = 0"
    huff = np.zeros((ncomp, 2, HUFF_BYTES), dtype=np.uint8)
    for c in range(ncomp):
        for cls, ident in ((0, seg[2 + 2 * c] >> 4), (1, 0x10 | (seg[2 + 2 * c] & 15))):
            if ident not in dht:
                return None, "a component's Huffman table is not defined"
            raw = dht[ident]
            huff[c, cls, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    # the entropy-coded data: FF 00 is data; FF D0 .. D7 split it; FF D9 ends it; anything else is not ours
    body = buf[i:]
    at = np.flatnonzero((body[:-1] == 0xFF) & (body[1:] != 0)) if body.shape[0] > 1 else np.zeros(0, dtype=np.int64)
    kinds = body[at + 1]
    end = n
    if at.size and kinds[-1] == 0xD9:
        end, at, kinds = i + int(at[-1]), at[:-1], kinds[:-1]      # whatever follows EOI is ignored, as decoders do
    elif at.size and (kinds == 0xD9).any():
        first = int(np.flatnonzero(kinds == 0xD9)[0])
        end, at, kinds = i + int(at[first]), at[:first], kinds[:first]
    if ((kinds < 0xD0) | (kinds > 0xD7)).any():
        return None, "a marker other than RSTn inside the scan (several scans, fill bytes or damage)"
    mcus = mcus_of(height, width, sampling)
    expected = -(-mcus // restart) - 1 if restart else 0
    if at.size != expected:
        return None, f"{at.size} restart markers, {expected} expected"
    if at.size and not np.array_equal(kinds & 7, np.arange(at.size) & 7):
        return None, "restart markers out of order"
    starts = np.concatenate(([i], i + at + 2)).astype(np.int64)
    ends = np.concatenate((i + at, [end])).astype(np.int64)
    per = restart if restart else mcus
    first = np.arange(starts.size, dtype=np.int64) * per
    segments = np.stack([starts, ends - starts, first, np.minimum(per, mcus - first)], axis=1)
    if int((ends - starts).max()) > SEGMENT_MAX_BYTES:
        return None, "a segment longer than 256 MiB"
    return JpegHeader(height, width, np.stack([dqt[c[2]] for c in comps]), huff, restart, (i, end), segments, sampling,
                      adobe is not None), None


@dataclass
class JpegPlan:
    """what dtk_jpeg_decode_coefficients_sampled / dtk_jpeg_pixels_sampled take for F files of one size and one sampling whose bytes
    lie one after the other"""
    frames: int
    height: int
    width: int
    segments: np.ndarray   # int64 [S, 5]: frame, byte offset in the stream, byte length, first MCU, MCU count
    huffman: np.ndarray    # uint8 [F, C, 2, 272] (C = 3 components, gray: 1)
    qtables: np.ndarray    # uint8 [F, C, 64]
    sampling: int = S420   # S420, S422, S444 or GRAY


def plan_jpeg(datas: Sequence, offsets: Optional[Sequence[int]] = None) -> Tuple[Optional[JpegPlan], Optional[str]]:
    """Parse every file with parse_jpeg; (plan, None) when all are eligible and of one size, else (None, "<index>: <reason>").
    offsets[f]: where file f starts in the stream the caller uploads (default: the files one after the other)."""
    return _plan(datas, offsets, parse_jpeg)


def plan_jpeg_sampled(datas: Sequence, offsets: Optional[Sequence[int]] = None) -> Tuple[Optional[JpegPlan], Optional[str]]:
    """plan_jpeg with parse_jpeg_sampled: all files must also be of ONE sampling, the plan's."""
    return _plan(datas, offsets, parse_jpeg_sampled)


def _plan(datas: Sequence, offsets: Optional[Sequence[int]], parse) -> Tuple[Optional[JpegPlan], Optional[str]]:
    if not len(datas):
        return None, "no files"
    headers: List[JpegHeader] = []
    for f, data in enumerate(datas):
        h, why = parse(data)
        if h is None:
            return None, f"file {f}: {why}"
        if headers and (h.height, h.width) != (headers[0].height, headers[0].width):
            return None, f"file {f}: {h.height} x {h.width}, file 0 is {headers[0].height} x {headers[0].width}"
        if headers and h.sampling != headers[0].sampling:
            return None, f"file {f}: sampling {SAMPLING_NAMES[h.sampling]}, file 0 is {SAMPLING_NAMES[headers[0].sampling]}"
        headers.append(h)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([len(d) for d in datas])))[:-1]
    segs = []
    for f, (h, off) in enumerate(zip(headers, offsets)):
        s = np.empty((h.segments.shape[0], 5), dtype=np.int64)
        s[:, 0], s[:, 1], s[:, 2:] = f, h.segments[:, 0] + int(off), h.segments[:, 1:]
        segs.append(s)
    return JpegPlan(len(headers), headers[0].height, headers[0].width, np.concatenate(segs),
                    np.stack([h.huffman for h in headers]), np.stack([h.qtables for h in headers]), headers[0].sampling), None


# ---- bytes: one pinned buffer, one upload --------------------------------------------------------------------------------------
Source = Union[str, os.PathLike, bytes, bytearray, memoryview]


def read_pinned(sources: Sequence[Source]) -> Tuple[torch.Tensor, List[np.ndarray]]:
    """All files' bytes in ONE pinned uint8 buffer, and a view of each file in it."""
    sizes = [len(s) if isinstance(s, (bytes, bytearray, memoryview)) else os.path.getsize(s) for s in sources]
    pinned = torch.empty(max(1, sum(sizes)), dtype=torch.uint8, pin_memory=True)
    whole = pinned.numpy()
    views, at = [], 0
    for s, n in zip(sources, sizes):
        view = whole[at:at + n]
        if isinstance(s, (bytes, bytearray, memoryview)):
            view[:] = np.frombuffer(s, dtype=np.uint8)
        else:
            with open(s, "rb") as fh:
                got = fh.readinto(memoryview(view))
            if got != n:
                raise OSError(f"{s}: read {got} of {n} bytes")
        views.append(view)
        at += n
    return pinned, views


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dino_tracker_amd: the JPEG decoder needs a GPU device -- the hot path has no CPU fallback")
    return device


ENTROPY_MODES = ("sequential", "parallel")


def entropy_mode(entropy: Optional[str] = None) -> str:
    """The entropy stage to use: `entropy` when given, else DTK_JPEG_ENTROPY, else "sequential" (one lane per segment:
    ops.jpeg_decode_coefficients).  "parallel": many lanes per segment (ops.jpeg_decode_coefficients_parallel, docs/JPEG_DECODE.md
    section 1b) -- the same coefficients and status.  ValueError on anything else.  Baseline files only: progressive files do not use it."""
    mode = os.environ.get("DTK_JPEG_ENTROPY", "sequential") if entropy is None else entropy
    if mode not in ENTROPY_MODES:
        raise ValueError(f"the JPEG entropy stage must be one of {ENTROPY_MODES} (argument `entropy` or DTK_JPEG_ENTROPY), got {mode!r}")
    return mode


def _entropy(pinned: torch.Tensor, plan: JpegPlan, device: torch.device, entropy: Optional[str] = None, subseq_bytes: int = 0):
    mode = entropy_mode(entropy)
    stream = pinned.to(device, non_blocking=True)
    huff = torch.from_numpy(plan.huffman).to(device)
    if mode == "parallel":
        return ops.jpeg_decode_coefficients_parallel(stream, plan.segments, huff, plan.height, plan.width, plan.sampling, subseq_bytes)
    return ops.jpeg_decode_coefficients(stream, plan.segments, huff, plan.height, plan.width, plan.sampling)


def _planned(sources: Sequence[Source]) -> Tuple[torch.Tensor, List[np.ndarray], JpegPlan]:
    pinned, views = read_pinned(sources)
    plan, why = plan_jpeg_sampled(views)
    if plan is None:
        raise ValueError(f"decode_jpeg: not decodable on the device -- {why}")
    return pinned, views, plan


def decode_jpeg_coefficients(sources: Sequence[Source], device="cuda:0", entropy: Optional[str] = None, subseq_bytes: int = 0
                             ) -> Tuple[torch.Tensor, torch.Tensor, JpegPlan]:
    """The entropy stage alone: (int16 [T, MCUs, B, 64] in zigzag order -- B = 6, 4, 3, 1 blocks per MCU for 4:2:0, 4:2:2, 4:4:4, gray --,
    int32 status [T] -- ops.JPEG_S_* bits --, the plan).  entropy, subseq_bytes: entropy_mode."""
    device = _device(device)
    pinned, _, plan = _planned(sources)
    coef, status = _entropy(pinned, plan, device, entropy, subseq_bytes)
    return coef, status, plan


def decode_planned(pinned: torch.Tensor, views: List[np.ndarray], plan: JpegPlan, device, fallback: bool = True,
                   with_status: bool = False, entropy: Optional[str] = None, subseq_bytes: int = 0):
    device = _device(device)
    coef, status = _entropy(pinned, plan, device, entropy, subseq_bytes)
    qt = torch.from_numpy(plan.qtables).to(device)
    out = ops.jpeg_pixels(coef, qt, plan.height, plan.width, status, plan.sampling)
    mode = "L" if plan.sampling == GRAY else "RGB"
    if plan.sampling == GRAY:
        out = out[..., None]
    host_status = status.cpu()                       # the one host read
    if fallback and bool(host_status.any()):
        from PIL import Image
        for f in torch.nonzero(host_status).flatten().tolist():
            with Image.open(io.BytesIO(views[f].tobytes())) as img:
                frame = np.asarray(img.convert(mode) if img.mode != mode else img)
            out[f] = torch.from_numpy(np.ascontiguousarray(frame).reshape(tuple(out.shape[1:]))).to(device)
    return (out, host_status) if with_status else out


def decode_jpeg(sources: Sequence[Source], device="cuda:0", fallback: bool = True, with_status: bool = False,
                entropy: Optional[str] = None, subseq_bytes: int = 0):
    """uint8 [T, H, W, 3] -- gray files: [T, H, W, 1] -- on `device` from JPEG files (paths) or byte strings of one size and one
    sampling.  ValueError with the reason when a file
    is not of the kind the device decodes (module docstring).  After the launches ONE host read, the frames' status; a frame
    whose status is not zero -- a damaged stream -- is decoded by Pillow instead and uploaded into its slot (`fallback`), which
    raises what Pillow raises.  with_status: also the int32 [T] status as the device reported it (host tensor).  entropy:
    "sequential" or "parallel" (default: DTK_JPEG_ENTROPY, else sequential), subseq_bytes: the parallel stage's sub-stream length
    (entropy_mode) -- the frames are the same either way."""
    pinned, views, plan = _planned(sources)
    return decode_planned(pinned, views, plan, device, fallback, with_status, entropy, subseq_bytes)


# ---- progressive files (SOF2): docs/JPEG_DECODE.md "Progressive files", csrc/jpeg_progressive.hip --------------------------------------
# Decoded on the device when asked for (decode_jpeg_progressive, DTK_JPEG_DECODE=device): 8 bit, components 1 2 3 with one of the
# three samplings above or one component, 8-bit quantisation tables before the first scan, Huffman coding, a legal and COMPLETE scan
# script.  parse_jpeg / parse_jpeg_sampled / plan_jpeg* / decode_jpeg keep refusing such files.
PROG_FIELDS = ops.JPEG_PROG_FIELDS
PROG_MAX_AL = 13


@dataclass
class JpegScan:
    components: Tuple[int, ...]  # indices into the frame's components (0: Y), in scan order: one, or (0, 1, 2) interleaved
    ss: int
    se: int
    ah: int
    al: int
    tables: Tuple[bytes, ...]    # the raw tables (272 bytes each) in force at the SOS: a DC first scan's DC table per component, an AC
    #                              scan's AC table, nothing for a DC refinement
    restart: int                 # the restart interval in force at the SOS, in units; 0: none
    segments: np.ndarray         # int64 [S, 4]: byte offset in the file, byte length, first unit, units -- a unit is an MCU of an
    #                              interleaved scan and a block of the component's real grid otherwise


@dataclass
class JpegProgressiveHeader:
    height: int
    width: int
    sampling: int
    qtables: np.ndarray          # uint8 [C, 64], zigzag order
    scans: List[JpegScan]
    adobe: bool = False

    @property
    def mcus(self) -> int:
        return mcus_of(self.height, self.width, self.sampling)


def scan_units(height: int, width: int, sampling: int, components: Sequence[int]) -> int:
    """what a scan's restart interval counts: the MCUs of an interleaved scan, else the blocks of the component's REAL grid,
    ceil(ceil(H v_c / v_max) / 8) rows of ceil(ceil(W h_c / h_max) / 8)"""
    if len(components) > 1:
        return mcus_of(height, width, sampling)
    _, _, mh, mw = ops.jpeg_geometry(sampling)
    if components[0] == 0:
        return -(-height // 8) * -(-width // 8)
    return -(-(-(-height // (mh // 8))) // 8) * -(-(-(-width // (mw // 8))) // 8)


def scan_levels(scans: Sequence) -> List[int]:
    """Scans i < j conflict when they share a component and their bands [ss, se] intersect: j reads or overwrites what i wrote.
    level(j) = 1 + the highest level among the earlier scans it conflicts with, 0 when there is none: scans of one level touch
    disjoint coefficients and may be decoded at the same time.  `scans`: objects with components, ss, se (JpegScan)."""
    levels: List[int] = []
    for j, b in enumerate(scans):
        level = 0
        for i in range(j):
            a = scans[i]
            if set(a.components) & set(b.components) and a.ss <= b.se and b.ss <= a.se:
                level = max(level, levels[i] + 1)
        levels.append(level)
    return levels


def parse_jpeg_progressive(data) -> Tuple[Optional[JpegProgressiveHeader], Optional[str]]:
    """Walk SOI .. EOI of one progressive file.  (header, None) when the device decodes it, else (None, why): not SOF2, a layout
    parse_jpeg_sampled would refuse in a baseline file too, a table or marker the walk cannot follow, a DQT behind the first SOS, an
    illegal succession of scans, or an INCOMPLETE progression (libjpeg smooths those: other pixels).  A DRI may stand before any
    SOS and holds from there on -- encoders that count the interval in rows write one per scan."""
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = int(buf.shape[0])
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        return None, "no SOI marker"
    # every FF that is not followed by 00: the markers, inside and outside the entropy-coded data
    marks = np.flatnonzero((buf[:-1] == 0xFF) & (buf[1:] != 0))
    dqt, dht, restart, sof, adobe = {}, {}, 0, None, None
    scans: List[JpegScan] = []
    geometry = None              # (height, width, ncomp, sampling, component ids' tables) once the SOF is read
    progress = None              # int [C, 64]: the Al each coefficient has reached, -1: not coded yet
    i = 2
    while True:
        if i + 2 > n or buf[i] != 0xFF:
            return None, f"no marker at byte {i}"
        marker = int(buf[i + 1])
        if marker == 0xFF:          # a fill byte
            i += 1
            continue
        if marker == 0xD9:
            break
        if marker == 0xC0:
            return None, "not progressive (baseline, SOF0)"
        if marker in _SOF_OTHERS and marker != 0xC2:
            return None, _SOF_OTHERS[marker]
        if marker == 0x01 or 0xD0 <= marker <= 0xD8 or marker == 0x00:
            return None, f"marker FF{marker:02X} between the segments"
        if i + 4 > n:
            return None, f"no marker at byte {i}"
        length = (int(buf[i + 2]) << 8) | int(buf[i + 3])
        if length < 2 or i + 2 + length > n:
            return None, f"segment FF{marker:02X} at byte {i} runs past the file"
        seg = bytes(buf[i + 4:i + 2 + length])
        i += 2 + length
        if marker == 0xDB:
            if scans:
                return None, "a DQT behind the first SOS"
            k = 0
            while k < len(seg):
                if seg[k] >> 4:
                    return None, "16-bit quantisation table"
                if (seg[k] & 15) > 3 or k + 65 > len(seg):
                    return None, "DQT: table id above 3, or the segment is short"
                dqt[seg[k] & 15] = np.frombuffer(seg[k + 1:k + 65], dtype=np.uint8)
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg) or (seg[k] >> 4) > 1 or (seg[k] & 15) > 3:
                    return None, "DHT: table class above 1, id above 3, or the segment is short"
                counts = list(seg[k + 1:k + 17])
                vals = seg[k + 17:k + 17 + sum(counts)]
                why = _check_huffman(seg[k] >> 4, counts, vals)      # an AC symbol (r << 4) with r <= 14 is an end-of-band run here
                if why:
                    return None, why
                raw = bytes(counts) + vals
                dht[seg[k]] = raw + bytes(HUFF_BYTES - len(raw))
                k += 17 + sum(counts)
        elif marker == 0xDD:
            if len(seg) != 2:
                return None, "DRI: wrong length"
            restart = (seg[0] << 8) | seg[1]
        elif marker == 0xEE:
            if seg[:5] == b"Adobe":
                adobe = seg[11] if len(seg) >= 12 else -1
        elif marker == 0xC2:
            if sof is not None:
                return None, "two SOF2 segments"
            sof = seg
            if len(sof) < 6:
                return None, "SOF2 is short"
            if sof[0] != 8:
                return None, f"{sof[0]}-bit samples"
            height, width, ncomp = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
            if ncomp not in (1, 3) or len(sof) != 6 + 3 * ncomp:
                return None, f"{ncomp} components"
            if height < 1 or width < 1:
                return None, "zero height or width (DNL)"
            comps = [(sof[6 + 3 * c], sof[7 + 3 * c], sof[8 + 3 * c]) for c in range(ncomp)]
            if [c[0] for c in comps] != [1, 2, 3][:ncomp]:
                return None, f"component ids {[c[0] for c in comps]}, not {'1 2 3' if ncomp == 3 else '1'}"
            factors = tuple(c[1] for c in comps)
            if ncomp == 1:
                sampling = GRAY
            elif factors in _FACTORS:
                sampling = _FACTORS[factors]
            else:
                return None, f"sampling {_FACTOR_NAMES.get(factors, [hex(v) for v in factors])}, not 4:2:0, 4:2:2 or 4:4:4"
            geometry = (height, width, ncomp, sampling, [c[2] for c in comps])
            progress = np.full((ncomp, 64), -1, dtype=np.int64)
        elif marker == 0xDA:
            if geometry is None:
                return None, "no SOF2 segment before the scan"
            height, width, ncomp, sampling, _ = geometry
            ns = seg[0] if seg else 0
            if ns < 1 or len(seg) != 4 + 2 * ns:
                return None, "SOS: wrong length"
            ids = [seg[1 + 2 * c] for c in range(ns)]
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            which = len(scans)
            if ns == 1:
                if not 1 <= ids[0] <= ncomp:
                    return None, f"scan {which}: component {ids[0]} is not in the frame"
                components = (ids[0] - 1,)
            elif ids == [1, 2, 3] and ncomp == 3:
                components = (0, 1, 2)
            else:
                return None, f"scan {which}: components {ids} interleaved, not 1 2 3"
            if ss > se or se > 63 or (ss == 0 and se != 0):
                return None, f"scan {which}: band {ss}-{se} is illegal (a DC scan has Ss = Se = 0)"
            if ss > 0 and ns != 1:
                return None, f"scan {which}: an AC scan of several components"
            if al > PROG_MAX_AL:
                return None, f"scan {which}: Al = {al} above {PROG_MAX_AL}"
            band = progress[list(components), ss:se + 1]
            if ah == 0:
                if (band != -1).any():
                    return None, f"scan {which}: a first scan (Ah = 0) of coefficients that are coded already"
            elif (band != ah).any() or al != ah - 1:
                return None, f"scan {which}: Ah/Al = {ah}/{al} is not the successor of what the band has reached"
            progress[list(components), ss:se + 1] = al
            tables: List[bytes] = []
            if ss == 0 and ah == 0:
                tables = [dht.get(seg[2 + 2 * c] >> 4) for c in range(ns)]
            elif ss > 0:
                tables = [dht.get(0x10 | (seg[2] & 15))]
            if any(t is None for t in tables):
                return None, f"scan {which}: a Huffman table is not defined"
            # the body: FF 00 is data, FF D0 .. D7 split it, any other marker ends it
            first = int(np.searchsorted(marks, i))
            k = first
            while k < marks.size and 0xD0 <= buf[marks[k] + 1] <= 0xD7:
                k += 1
            if k == marks.size:
                return None, f"scan {which}: the file ends inside the scan"
            end = int(marks[k])
            at = marks[first:k].astype(np.int64)
            units = scan_units(height, width, sampling, components)
            expected = -(-units // restart) - 1 if restart else 0
            if at.size != expected:
                return None, f"scan {which}: {at.size} restart markers, {expected} expected"
            if at.size and not np.array_equal(buf[at + 1] & 7, np.arange(at.size) & 7):
                return None, f"scan {which}: restart markers out of order"
            starts = np.concatenate(([i], at + 2)).astype(np.int64)
            ends = np.concatenate((at, [end])).astype(np.int64)
            if int((ends - starts).max()) > SEGMENT_MAX_BYTES:
                return None, "a segment longer than 256 MiB"
            per = restart if restart else units
            first_unit = np.arange(starts.size, dtype=np.int64) * per
            segments = np.stack([starts, ends - starts, first_unit, np.minimum(per, units - first_unit)], axis=1)
            scans.append(JpegScan(components, ss, se, ah, al, tuple(tables), restart, segments))
            i = end
        # COM, APPn and anything else with a length: skipped
    if geometry is None:
        return None, "no SOF2 segment"
    if not scans:
        return None, "no scan"
    height, width, ncomp, sampling, tq = geometry
    if adobe is not None and (ncomp != 3 or adobe != 1):
        return None, (f"Adobe APP14 segment on {ncomp} component" if ncomp != 3 else
                      f"Adobe APP14 segment with transform {adobe}, not 1 (YCbCr)" if adobe >= 0 else "Adobe APP14 segment is short")
    if any(t not in dqt for t in tq):
        return None, "a component's quantisation table is not defined"
    if (progress != 0).any():
        c, k = (int(v[0]) for v in np.nonzero(progress != 0))
        return None, (f"incomplete progression: coefficient {k} of component {c + 1} " +
                      ("is never coded" if progress[c, k] < 0 else f"stops at Al = {int(progress[c, k])}"))
    return JpegProgressiveHeader(height, width, sampling, np.stack([dqt[t] for t in tq]), scans, adobe is not None), None


@dataclass
class JpegProgressivePlan:
    """what dtk_jpeg_decode_progressive / dtk_jpeg_pixels_sampled take for F progressive files of one size and one sampling"""
    frames: int
    height: int
    width: int
    segments: np.ndarray   # int64 [S, 14], ordered by level: the rows include/dtk.h documents
    tables: np.ndarray     # uint8 [N, 272]: every distinct raw Huffman table the rows name
    qtables: np.ndarray    # uint8 [F, C, 64]
    sampling: int


def plan_jpeg_progressive(datas: Sequence, offsets: Optional[Sequence[int]] = None
                          ) -> Tuple[Optional[JpegProgressivePlan], Optional[str]]:
    """Parse every file with parse_jpeg_progressive; (plan, None) when all are eligible and of one size and one sampling, else
    (None, "file <index>: <reason>").  Every frame may have its own scan script and tables; the levels are scan_levels' per frame."""
    if not len(datas):
        return None, "no files"
    headers: List[JpegProgressiveHeader] = []
    for f, data in enumerate(datas):
        h, why = parse_jpeg_progressive(data)
        if h is None:
            return None, f"file {f}: {why}"
        if headers and (h.height, h.width) != (headers[0].height, headers[0].width):
            return None, f"file {f}: {h.height} x {h.width}, file 0 is {headers[0].height} x {headers[0].width}"
        if headers and h.sampling != headers[0].sampling:
            return None, f"file {f}: sampling {SAMPLING_NAMES[h.sampling]}, file 0 is {SAMPLING_NAMES[headers[0].sampling]}"
        headers.append(h)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([len(d) for d in datas])))[:-1]
    index, rows = {}, []
    for f, (h, off) in enumerate(zip(headers, offsets)):
        for scan, level in zip(h.scans, scan_levels(h.scans)):
            if level > 255:
                return None, f"file {f}: more than 256 levels of scans"
            t = [index.setdefault(raw, len(index)) for raw in scan.tables] + [0, 0, 0]
            r = np.empty((scan.segments.shape[0], PROG_FIELDS), dtype=np.int64)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3] = f, scan.segments[:, 0] + int(off), scan.segments[:, 1], level
            r[:, 4:8] = (scan.ss, scan.se, scan.ah, scan.al)
            r[:, 8] = scan.components[0] if len(scan.components) == 1 else -1
            r[:, 9:11], r[:, 11:14] = scan.segments[:, 2:4], t[:3]
            rows.append(r)
    rows = np.concatenate(rows)
    rows = np.ascontiguousarray(rows[np.argsort(rows[:, 3], kind="stable")])
    tables = np.zeros((max(1, len(index)), HUFF_BYTES), dtype=np.uint8)
    for raw, at in index.items():
        tables[at] = np.frombuffer(raw, dtype=np.uint8)
    return JpegProgressivePlan(len(headers), headers[0].height, headers[0].width, rows, tables,
                               np.stack([h.qtables for h in headers]), headers[0].sampling), None


def _planned_progressive(sources: Sequence[Source]) -> Tuple[torch.Tensor, List[np.ndarray], JpegProgressivePlan]:
    pinned, views = read_pinned(sources)
    plan, why = plan_jpeg_progressive(views)
    if plan is None:
        raise ValueError(f"decode_jpeg_progressive: not decodable on the device -- {why}")
    return pinned, views, plan


def _entropy_progressive(pinned: torch.Tensor, plan: JpegProgressivePlan, device: torch.device):
    stream = pinned.to(device, non_blocking=True)
    tables = torch.from_numpy(plan.tables).to(device)
    return ops.jpeg_decode_progressive(stream, plan.segments, tables, plan.frames, plan.height, plan.width, plan.sampling)


def decode_jpeg_progressive_coefficients(sources: Sequence[Source], device="cuda:0"
                                         ) -> Tuple[torch.Tensor, torch.Tensor, JpegProgressivePlan]:
    """The entropy stage of progressive files alone: (int16 [T, MCUs, B, 64] zigzag -- decode_jpeg_coefficients' layout: what the
    baseline file of the same picture holds --, int32 status [T], the plan)."""
    device = _device(device)
    pinned, _, plan = _planned_progressive(sources)
    coef, status = _entropy_progressive(pinned, plan, device)
    return coef, status, plan


def decode_planned_progressive(pinned: torch.Tensor, views: List[np.ndarray], plan: JpegProgressivePlan, device, fallback: bool = True,
                               with_status: bool = False):
    """decode_planned for a progressive plan: the scans level by level, then the pixel stage of the baseline decoder, unchanged."""
    device = _device(device)
    coef, status = _entropy_progressive(pinned, plan, device)
    qt = torch.from_numpy(plan.qtables).to(device)
    out = ops.jpeg_pixels(coef, qt, plan.height, plan.width, status, plan.sampling)
    mode = "L" if plan.sampling == GRAY else "RGB"
    if plan.sampling == GRAY:
        out = out[..., None]
    host_status = status.cpu()                       # the one host read
    if fallback and bool(host_status.any()):
        from PIL import Image
        for f in torch.nonzero(host_status).flatten().tolist():
            with Image.open(io.BytesIO(views[f].tobytes())) as img:
                frame = np.asarray(img.convert(mode) if img.mode != mode else img)
            out[f] = torch.from_numpy(np.ascontiguousarray(frame).reshape(tuple(out.shape[1:]))).to(device)
    return (out, host_status) if with_status else out


def decode_jpeg_progressive(sources: Sequence[Source], device="cuda:0", fallback: bool = True, with_status: bool = False):
    """decode_jpeg for PROGRESSIVE files (paths or byte strings) of one size and one sampling: uint8 [T, H, W, 3] -- gray files:
    [T, H, W, 1] -- on `device`.  ValueError with the reason when a file is not of the kind parse_jpeg_progressive accepts.  The same
    contract otherwise: ONE host read, the frames' status, and Pillow for a frame whose status is not zero (`fallback`)."""
    pinned, views, plan = _planned_progressive(sources)
    return decode_planned_progressive(pinned, views, plan, device, fallback, with_status)
