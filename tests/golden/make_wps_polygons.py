"""Extract the drill geometries of the reference's WPS acceptance requests
(acceptance_tests/polygon_requests/*.xml and *.payload of chuc92man/gsky:
32 Australian local-government areas plus the two sample payloads) into
tests/golden/wps_polygons.<k>.json.gz: {file name: GeoJSON text of the
wps:ComplexData geometry input}, unchanged, dealt in file-name order over as
few parts as keep each under PART_LIMIT bytes.  Data only (the requests' inputs);
run in the build container, where /root/reference exists:

    python tests/golden/make_wps_polygons.py [/root/reference]
"""
import glob
import gzip
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PART_LIMIT = 1000 * 1000   # committed files stay under 1 MiB


def pack(part):
    return gzip.compress(json.dumps(part).encode("utf-8"), 9, mtime=0)


def write_parts(out):
    """Consecutive runs of the sorted entries, each run as long as its
    compressed part stays under PART_LIMIT."""
    parts = [{}]
    for name in sorted(out):
        if parts[-1] and len(pack({**parts[-1], name: out[name]})) > PART_LIMIT:
            parts.append({})
        parts[-1][name] = out[name]
    for old in glob.glob(os.path.join(HERE, "wps_polygons.*json.gz")):
        os.remove(old)
    for k, part in enumerate(parts):
        with open(os.path.join(HERE, "wps_polygons.%d.json.gz" % k), "wb") as f:
            f.write(pack(part))
    return len(parts)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    for p in sorted(glob.glob(os.path.join(ref, "acceptance_tests", "polygon_requests", "*"))):
        txt = open(p, encoding="utf-8").read()
        m = re.search(r"<ows:Identifier>geometry</ows:Identifier>.*?<wps:ComplexData[^>]*>(.*?)</wps:ComplexData>",
                      txt, re.S)
        if not m:
            continue
        geo = m.group(1).strip()
        json.loads(geo)   # must be valid GeoJSON text
        out[os.path.basename(p)] = geo
    print("%d geometries in %d parts" % (len(out), write_parts(out)))


if __name__ == "__main__":
    main()
