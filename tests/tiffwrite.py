"""The small TIFF writer of tests/test_ingest.py, copied for the device-decode
tests and extended by what they need: compression 32946 (the old Deflate
code), predictor 3 (floating point), a Deflate level and a hook that damages
one block's stream.  Classic / BigTIFF, either byte order, tiles or strips,
chunky or planar, internal overviews."""
import struct
import zlib

import numpy as np


# ---------------------------------------------------------------- a small TIFF writer
def _packbits(b: bytes) -> bytes:
    out, i = bytearray(), 0
    while i < len(b):
        j = i
        while j + 1 < len(b) and b[j + 1] == b[i] and j - i < 127:
            j += 1
        if j > i:
            out += bytes([(257 - (j - i + 1)) & 0xFF, b[i]])
            i = j + 1
        else:
            k = i
            while k < len(b) and k - i < 128 and not (k + 1 < len(b) and b[k + 1] == b[k]):
                k += 1
            k = max(k, i + 1)
            out += bytes([k - i - 1]) + b[i:k]
            i = k
    return bytes(out)


def _predict(block: np.ndarray, predictor: int) -> np.ndarray:
    """block (rows, cols, samples) -> the bytes the predictor stores."""
    if predictor == 2:
        if block.dtype.kind == "f":   # differences of the samples' bit patterns, as for integers
            u = block.astype(block.dtype.newbyteorder("=")).view("u%d" % block.dtype.itemsize)
            d = u.copy()
            d[:, 1:] = u[:, 1:] - u[:, :-1]
            return d.astype(d.dtype.newbyteorder(block.dtype.byteorder))
        d = block.copy()
        d[:, 1:] = block[:, 1:] - block[:, :-1]   # wraps in the sample type
        return d
    if predictor == 3:
        # floating point (TIFF Technical Note 3): per row the byte planes of
        # the samples, most significant first, then byte differences `samples`
        # apart
        rows, cols, samples = block.shape
        es = block.dtype.itemsize
        le = np.ascontiguousarray(block.astype(block.dtype.newbyteorder("<"))).view(np.uint8)
        le = le.reshape(rows, cols * samples, es)
        planes = le[:, :, ::-1].transpose(0, 2, 1).reshape(rows, es * cols * samples)
        d = planes.copy()
        d[:, samples:] = planes[:, samples:] - planes[:, :-samples]
        return d
    return block


def write_tiff(path, planes, tile=None, rows_per_strip=None, compression=1, predictor=1, big=False, be=False,
               planar=2, geo=None, nodata=None, overviews=(), level=6, mangle=None):
    """planes: list of 2-D arrays (bands) of one dtype; overviews: list of
    lists of planes written as reduced-resolution IFDs after the first.
    compression 8 and 32946 deflate at `level`; mangle(i, stream) may replace
    the stored stream of block i (to write a damaged file)."""
    bo = ">" if be else "<"
    dt = planes[0].dtype
    fmt = {"u": 1, "i": 2, "f": 3}[dt.kind]
    out = bytearray(b"MM" if be else b"II")
    out += struct.pack(bo + "H", 43 if big else 42)
    if big:
        out += struct.pack(bo + "HHQ", 8, 0, 0)
    else:
        out += struct.pack(bo + "I", 0)
    first_ptr = 8 if big else 4
    prev_next_ptr = first_ptr
    levels = [planes] + [list(o) for o in overviews]
    for lvl, bands in enumerate(levels):
        h, w = bands[0].shape
        nb = len(bands)
        if tile:
            tw, th = tile
            across, down = -(-w // tw), -(-h // th)
        else:
            tw, th = w, rows_per_strip or h
            across, down = 1, -(-h // th)
        chunks = []
        arr = np.stack(bands, -1).astype(dt.newbyteorder(">" if be else "<"))
        groups = [[b] for b in range(nb)] if planar == 2 else [list(range(nb))]
        for grp in groups:
            for by in range(down):
                for bx in range(across):
                    if tile:
                        blk = np.zeros((th, tw, len(grp)), arr.dtype)
                        src = arr[by * th:(by + 1) * th, bx * tw:(bx + 1) * tw][..., grp]
                        blk[:src.shape[0], :src.shape[1]] = src
                    else:
                        blk = arr[by * th:(by + 1) * th][..., grp]
                    raw = _predict(blk, predictor).tobytes()
                    c = (zlib.compress(raw, level) if compression in (8, 32946) else
                         _packbits(raw) if compression == 32773 else raw)
                    chunks.append(mangle(len(chunks), c) if mangle else c)
        offs = []
        for c in chunks:
            offs.append(len(out))
            out += c
            if len(out) % 2:
                out += b"\0"
        ents = []   # (tag, type, values)
        ents.append((254, 4, [1 if lvl else 0]))
        ents.append((256, 4, [w]))
        ents.append((257, 4, [h]))
        ents.append((258, 3, [dt.itemsize * 8] * nb))
        ents.append((259, 3, [compression]))
        ents.append((262, 3, [1]))
        if not tile:
            ents.append((273, 16 if big else 4, offs))
        ents.append((277, 3, [nb]))
        if not tile:
            ents.append((278, 4, [th]))
            ents.append((279, 16 if big else 4, [len(c) for c in chunks]))
        ents.append((284, 3, [planar]))
        if predictor != 1:
            ents.append((317, 3, [predictor]))
        if tile:
            ents.append((322, 3, [tw]))
            ents.append((323, 3, [th]))
            ents.append((324, 16 if big else 4, offs))
            ents.append((325, 16 if big else 4, [len(c) for c in chunks]))
        ents.append((339, 3, [fmt] * nb))
        if geo and lvl == 0:
            for tag, typ, vals in geo:
                ents.append((tag, typ, vals))
        if nodata is not None and lvl == 0:
            ents.append((42113, 2, nodata))
        ents.sort()
        ifd_off = len(out)
        out[prev_next_ptr:prev_next_ptr + (8 if big else 4)] = struct.pack(bo + ("Q" if big else "I"), ifd_off)
        esz, inl = (20, 8) if big else (12, 4)
        body = bytearray(struct.pack(bo + ("Q" if big else "H"), len(ents)))
        extra = bytearray()
        extra_base = ifd_off + len(body) + esz * len(ents) + (8 if big else 4)
        tcode = {2: "s", 3: "H", 4: "I", 12: "d", 16: "Q"}
        tsize = {2: 1, 3: 2, 4: 4, 12: 8, 16: 8}
        for tag, typ, vals in ents:
            if typ == 2:
                data = vals.encode() + b"\0"
                cnt = len(data)
            else:
                data = struct.pack(bo + "%d%s" % (len(vals), tcode[typ]), *vals)
                cnt = len(vals)
            ent = struct.pack(bo + ("HHQ" if big else "HHI"), tag, typ, cnt)
            if len(data) <= inl:
                ent += data + b"\0" * (inl - len(data))
            else:
                ent += struct.pack(bo + ("Q" if big else "I"), extra_base + len(extra))
                extra += data
                if len(extra) % 2:
                    extra += b"\0"
            body += ent
        prev_next_ptr = ifd_off + len(body)
        body += b"\0" * (8 if big else 4)
        out += body + extra
    with open(path, "wb") as f:
        f.write(bytes(out))


def geokeys(model=1, raster=1, keys=()):
    """GeoKeyDirectory: (key, value) SHORT keys after GTModelType / GTRasterType."""
    ks = [(1024, model), (1025, raster)] + list(keys)
    vals = [1, 1, 0, len(ks)]
    for k, v in ks:
        vals += [k, 0, 1, v]
    return (34735, 3, vals)
