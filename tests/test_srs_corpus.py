"""CPU test of the SRS parser against tests/golden/srs_corpus.json.gz: every
string of the corpus (tests/make_srs_corpus.py) gives the return code the
fixture's commit gave and, where that is 0, the same gskyhip_crs to the last
bit.  After an error only the code is compared (include/gskyhip.h promises
nothing about the struct then).  No kernel is launched."""
import ctypes
import gzip
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _first_difference(got, exp):
    from gsky_amd import _lib
    for name, _ in _lib.Crs._fields_:
        f = getattr(_lib.Crs, name)
        if got[f.offset:f.offset + f.size] != exp[f.offset:f.offset + f.size]:
            a, b = _lib.Crs.from_buffer_copy(got), _lib.Crs.from_buffer_copy(exp)
            va, vb = getattr(a, name), getattr(b, name)
            if not isinstance(va, (int, float)):
                va, vb = list(va), list(vb)
            return "%s: %r, recorded %r" % (name, va, vb)
    return "padding bytes"


def test_srs_corpus_replays_bit_for_bit():
    from gsky_amd import _lib
    L = _lib.lib()
    doc = json.loads(gzip.open(os.path.join(HERE, "golden", "srs_corpus.json.gz")).read().decode("utf-8"))
    assert doc["struct_size"] == ctypes.sizeof(_lib.Crs) == 352
    assert len(doc["commit"]) == 40
    assert len(doc["cases"]) >= 250
    bad = []
    for srs, rc, raw in doc["cases"]:
        c = _lib.Crs()
        got = L.gskyhip_crs_from_srs(srs.encode(), ctypes.byref(c))
        if got != rc:
            bad.append("%r: returned %d, recorded %d" % (srs, got, rc))
        elif rc == 0 and bytes(c) != bytes.fromhex(raw):
            bad.append("%r: %s" % (srs, _first_difference(bytes(c), bytes.fromhex(raw))))
    assert not bad, "%d of %d strings differ from commit %s:\n%s" % (len(bad), len(doc["cases"]), doc["commit"][:12],
                                                                    "\n".join(bad[:20]))
