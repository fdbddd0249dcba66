"""Record the bytes of the two Deflate encoders into
tests/golden/png_streams.json, so that a later change of their code is tied
to the bytes of the commit the record was made from:

  "png": for every case of tests/test_png_deflate.py's CASES but rows_4097
      (host zlib: its bytes are the installed zlib's), in modes "default" and
      "fixed" (GSKYHIP_PNG_FIXED=1), per tile the length and the SHA-256 of
      the zlib stream (the concatenated IDAT payloads) gskyhip_encode_png
      gives on the GPU;
  "deflate_host": for every block of tests/deflate_corpus.py, as a zlib and
      as a raw stream at levels 0 and 6, the same of
      gskyhip_deflate_blocks_host (no GPU needed);
  "commit": the commit the library was built from.

Data only.  Run from the repository root with the library built, on a machine
with a HIP device (--no-gpu keeps the "png" records of the existing file):

    python tests/golden/make_png_streams.py COMMIT [--out FILE] [--no-gpu]
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PNG_MODES = {"default": None, "fixed": "GSKYHIP_PNG_FIXED"}
DEFLATE_MODES = {"zlib6": (True, 6), "raw6": (False, 6), "zlib0": (True, 0), "raw0": (False, 0)}


def record(stream):
    return {"len": len(stream), "sha256": hashlib.sha256(stream).hexdigest()}


def png_records():
    import torch

    from gsky_amd.encode import encode_png
    from tests.test_png import _chunks
    from tests.test_png_deflate import CASES, pack, tiles_of
    out = {}
    for mode, var in PNG_MODES.items():
        os.environ.pop("GSKYHIP_PNG_FIXED", None)
        os.environ.pop("GSKYHIP_PNG_ZLIB", None)
        if var:
            os.environ[var] = "1"
        out[mode] = {}
        for name in CASES:
            if name == "rows_4097":
                continue
            batch, sizes = pack(tiles_of(name))
            pngs = encode_png(torch.from_numpy(batch).to("cuda:0"), sizes)
            out[mode][name] = [record(b"".join(d for t, d in _chunks(p) if t == b"IDAT")) for p in pngs]
    os.environ.pop("GSKYHIP_PNG_FIXED", None)
    return out


def deflate_host_records():
    from gsky_amd import encode
    from tests.deflate_corpus import corpus
    names, blocks = [n for n, _ in corpus()], [b for _, b in corpus()]
    out = {}
    for mode, (wrapper, level) in DEFLATE_MODES.items():
        streams = encode.deflate_blocks(blocks, zlib_wrapper=wrapper, level=level, where="host")
        out[mode] = [dict(record(z), name=n) for n, z in zip(names, streams)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("commit")
    ap.add_argument("--out", default=os.path.join(HERE, "png_streams.json"))
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    path = a.out
    doc = {"commit": a.commit}
    if a.no_gpu:
        doc["png"] = json.load(open(os.path.join(HERE, "png_streams.json")))["png"]
    else:
        doc["png"] = png_records()
    doc["deflate_host"] = deflate_host_records()
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d png records, %d deflate records" % (
        path, sum(len(v) for m in doc["png"].values() for v in m.values()),
        sum(len(v) for v in doc["deflate_host"].values())))


if __name__ == "__main__":
    main()
