"""What the KITTI flow evaluation is checked against, none of it the project's own code:

  - a float64 restatement of of_flow_eval / of_flow_upsample (include/oflow.h): the half-pixel
    bilinear upsampling with border replication, the scaling to native pixels, the devkit's
    decode of the 16-bit map, the end-point error and the 3 px / 5 % outlier rule;
  - an independent PNG writer and reader for 8- and 16-bit RGB (zlib + struct; the writer with
    any of the five row filters, or cycling them, and Adam7 interlacing; the reader for
    non-interlaced files with any filter), so the project's decoder and encoder are each
    checked against something that is not the other;
  - the test inputs: flows and ground-truth maps on which neither threshold of the outlier rule
    ever decides within rounding.
"""
import struct
import zlib

import numpy as np

# ---- independent PNG writer / reader ----------------------------------------------------------
_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filter_rows(rows, bpp, filt):
    """rows: (h, rb) uint8 -> the filtered scanlines with their type bytes.  filt 0-4, or "cycle"
    (row y uses filter y % 5)."""
    h, rb = rows.shape
    out = bytearray()
    prev = [0] * rb
    for y in range(h):
        cur = rows[y].tolist()
        t = y % 5 if filt == "cycle" else filt
        line = bytearray(rb)
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]
            line[i] = (cur[i] - pred) & 255
        out.append(t)
        out += line
        prev = cur
    return bytes(out)


def png_bytes(img, filt=0, interlace=False, depth=None, ctype=2):
    """An RGB image (h, w, 3), uint8 or uint16, as PNG file bytes (colour type 2, depth 8 / 16,
    big-endian samples); ``ctype=0`` writes a (h, w) gray image instead."""
    img = np.asarray(img)
    depth = depth or (16 if img.dtype == np.uint16 else 8)
    assert img.dtype == (np.uint16 if depth == 16 else np.uint8)
    h, w = img.shape[:2]
    ch = 3 if ctype == 2 else 1
    assert img.reshape(h, w, -1).shape[2] == ch
    bpp = ch * depth // 8

    def rows_of(sub):
        hh, ww = sub.shape[:2]
        be = sub.astype(">u2" if depth == 16 else np.uint8)
        return np.frombuffer(be.tobytes(), np.uint8).reshape(hh, ww * bpp)

    if interlace:
        x0, y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
        dx, dy = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)
        raw = b""
        for p in range(7):
            sub = img[y0[p]::dy[p], x0[p]::dx[p]]
            if sub.shape[0] and sub.shape[1]:
                raw += _filter_rows(rows_of(sub), bpp, filt)
    else:
        raw = _filter_rows(rows_of(img), bpp, filt)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if interlace else 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b"")


def write_png(path, img, filt=0, interlace=False):
    with open(path, "wb") as f:
        f.write(png_bytes(img, filt, interlace))


def read_png(path):
    """A non-interlaced RGB PNG of depth 8 or 16 -> ((h, w, 3) uint8 / uint16, the list of the
    rows' filter types)."""
    data = open(path, "rb").read()
    assert data[:8] == _SIG
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = head
    assert ctype == 2 and depth in (8, 16) and interlace == 0, head
    bpp = 3 * depth // 8
    rb = w * bpp
    raw = zlib.decompress(idat)
    assert len(raw) == h * (rb + 1)
    rows, filters = [], []
    prev = [0] * rb
    for y in range(h):
        t = raw[y * (rb + 1)]
        line = list(raw[y * (rb + 1) + 1:(y + 1) * (rb + 1)])
        for i in range(rb):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            line[i] = (line[i] + (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]) & 255
        rows.append(line)
        filters.append(t)
        prev = line
    arr = np.array(rows, np.uint8).reshape(h, rb)
    if depth == 16:
        arr = np.frombuffer(arr.tobytes(), ">u2").astype(np.uint16)
    return arr.reshape(h, w, 3), filters


# ---- float64 restatement ----------------------------------------------------------------------
def upsample_np(flow, gh, gw):
    """(fh, fw, 2) on its own grid -> (gh, gw, 2) float64 in pixels of the gh x gw image."""
    f = np.asarray(flow, np.float64)
    fh, fw = f.shape[:2]

    def axis(g, n):
        s = np.clip((np.arange(g) + 0.5) * n / g - 0.5, 0.0, n - 1.0)
        i0 = np.floor(s).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), s - i0

    y0, y1, fy = axis(gh, fh)
    x0, x1, fx = axis(gw, fw)
    fx, fy = fx[None, :, None], fy[:, None, None]
    p00, p01 = f[y0][:, x0], f[y0][:, x1]
    p10, p11 = f[y1][:, x0], f[y1][:, x1]
    top = p00 + (p01 - p00) * fx
    bot = p10 + (p11 - p10) * fx
    val = top + (bot - top) * fy
    return val * np.array([gw / fw, gh / fh])


def decode_np(rgb):
    """(h, w, 3) uint16 -> (ground truth (h, w, 2) float64, valid bool): the KITTI devkit."""
    rgb = np.asarray(rgb)
    return (rgb[:, :, :2].astype(np.float64) - 32768.0) / 64.0, rgb[:, :, 2] != 0


def epe_np(uv, rgb):
    """Per pixel: (epe, |ground truth|, valid, outlier) of a native-size flow uv (h, w, 2)."""
    gt, valid = decode_np(rgb)
    epe = np.sqrt(((np.asarray(uv, np.float64) - gt) ** 2).sum(-1))
    mag = np.sqrt((gt ** 2).sum(-1))
    return epe, mag, valid, valid & (epe > 3.0) & (epe > 0.05 * mag)


def flow_eval_np(flow, maps):
    """of_flow_eval in float64: (sum_epe (n,), n_valid (n,), n_outlier (n,))."""
    s, v, o = [], [], []
    for f, rgb in zip(flow, maps):
        epe, _, valid, outlier = epe_np(upsample_np(f, rgb.shape[0], rgb.shape[1]), rgb)
        s.append(epe[valid].sum())
        v.append(int(valid.sum()))
        o.append(int(outlier.sum()))
    return np.array(s), np.array(v, np.int64), np.array(o, np.int64)


def margins_np(flow, maps):
    """Over every valid pixel of the batch: (min |epe - 3|, min |epe / |gt| - 0.05|); (inf, inf)
    without a valid pixel.  A valid pixel with a zero ground-truth vector has an infinite ratio
    when epe > 0 and none (NaN: the margin then fails) when epe = 0."""
    m3, m5 = np.inf, np.inf
    for f, rgb in zip(flow, maps):
        epe, mag, valid, _ = epe_np(upsample_np(f, rgb.shape[0], rgb.shape[1]), rgb)
        if valid.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = epe[valid] / mag[valid]
            d5 = np.abs(ratio - 0.05)
            m3 = min(m3, np.abs(epe[valid] - 3.0).min())
            m5 = np.nan if np.isnan(d5).any() else min(m5, d5.min())
    return m3, m5


# ---- inputs -----------------------------------------------------------------------------------
SMALL_ERR = np.array([0.0, 0.25, 1.0, 2.5, 3.5, 6.0, 20.0])
LARGE_ERR = np.array([0.0, 0.25, 4.0, 20.0])


def make_flow(fh, fw, gh, gw, rng):
    """A float32 (fh, fw, 2) flow on its own grid whose native magnitude is in [0, 30] px in the
    left half and [110, 190] px in the right half, each half with a direction of its own
    +-0.2 rad."""
    right = ((np.arange(fw) + 0.5) / fw >= 0.5)[None, :]
    mag = np.where(right, rng.uniform(110.0, 190.0, (fh, fw)), rng.uniform(0.0, 30.0, (fh, fw)))
    base = rng.uniform(0.0, 2 * np.pi, 2)
    ang = np.where(right, base[1], base[0]) + rng.uniform(-0.2, 0.2, (fh, fw))
    native = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    return (native * np.array([fw / gw, fh / gh])).astype(np.float32)


def make_gt(up, rng, keep=0.6):
    """A ground-truth map (h, w, 3) uint16 for the float64 native-size flow ``up``.

    Valid only where |up| <= 40 (the small class) or 100 <= |up| <= 200 (the large class; the
    blend band between a flow's halves is invalid), thinned to about ``keep``.  Ground truth =
    up + an error vector of random direction whose magnitude is drawn from SMALL_ERR / LARGE_ERR
    by class, quantised to 1/64: errors below 3 px, above it and outliers, above it but within
    5 % of a large ground truth.  So that neither threshold decides within rounding, a pixel
    whose quantised result lies within 0.25 px of the 3 px threshold or within 5e-3 of the 5 %
    ratio (or has a zero ground-truth vector) draws again, up to eight times.  The redraw does
    real work -- a 1 px error on a 20 px ground truth is a ratio of exactly 0.05 -- and its
    cut-off is what sets the observed 5 % margin (5.0e-3 on the test's shapes; the 3 px margin,
    0.49 px, comes from the error magnitudes themselves).  No pixel is dropped for it: one that
    still lies near a threshold after eight draws raises AssertionError, so the test fails on
    its input."""
    h, w = up.shape[:2]
    mag = np.sqrt((up ** 2).sum(-1))
    small, large = mag <= 40.0, (mag >= 100.0) & (mag <= 200.0)
    valid = (small | large) & (rng.uniform(size=(h, w)) < keep)
    q = np.zeros((h, w, 2))
    redo = valid.copy()
    for _ in range(8):
        k = int(redo.sum())
        if k == 0:
            break
        m = np.where(small[redo], rng.choice(SMALL_ERR, k), rng.choice(LARGE_ERR, k))
        a = rng.uniform(0.0, 2 * np.pi, k)
        q[redo] = np.rint((up[redo] + np.stack([m * np.cos(a), m * np.sin(a)], -1)) * 64.0) / 64.0
        epe = np.sqrt(((up - q) ** 2).sum(-1))
        gm = np.sqrt((q ** 2).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            near = (np.abs(epe - 3.0) < 0.25) | ~(np.abs(epe / gm - 0.05) >= 5e-3) | (gm == 0)
        redo = valid & near
    assert not redo.any(), "%d pixels near a threshold after eight draws" % int(redo.sum())
    rgb = np.zeros((h, w, 3), np.uint16)
    rgb[:, :, :2] = np.where(valid[:, :, None], np.clip(q * 64.0 + 32768.0, 0, 65535), 0)
    rgb[:, :, 2] = valid
    return rgb


def make_case(fh, fw, sizes, seed):
    """One batch: flow float32 (n, fh, fw, 2) and its n ground-truth maps of the given sizes."""
    rng = np.random.default_rng(seed)
    flows, maps = [], []
    for gh, gw in sizes:
        f = make_flow(fh, fw, gh, gw, rng)
        flows.append(f)
        maps.append(make_gt(upsample_np(f, gh, gw), rng))
    return np.stack(flows), maps
