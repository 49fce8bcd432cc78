#!/usr/bin/env python3
"""Writes tests/golden/snf_params_vectors.json: [length, SHA-256] of every input and of what the pure-Python SnappyFramedOutputStream (tests/snf_params_ref.py) makes of every input of
tests/snf_params_cases.py at every parameter set the tests use -- the catalog, and the constructed pairs at the ratio's edge.  The file pins the model: the GPU tests
take their expected bytes from it, so a change to the model that changes an output has to show here (tests/test_snf_params_ref.py compares).
Run after a deliberate change to the model or the cases:   python tools/record_snf_params_vectors.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import snf_params_cases as cases, snf_params_ref as ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "snf_params_vectors.json")


def entry(out):
    """[length, SHA-256]"""
    return [len(out), hashlib.sha256(out).hexdigest()]


def vectors():
    inputs = {str(b): {name: entry(data) for name, data in cases.inputs(b)} for b in cases.BLOCK_SIZES}  # the inputs, once per block size: a changed input shows here
    catalog = {cases.params_name(p): {name: entry(cases.expected(p, name)) for name, _ in cases.inputs(p[1])} for p in cases.parameter_sets()}
    pairs = {name: {"input": entry(data), "kept": entry(ref.compress(data, True, block_size, kept)), "raw": entry(ref.compress(data, True, block_size, raw)),
                    "ratio_bits": [ref.ratio_bits(kept), ref.ratio_bits(raw)]}
             for name, block_size, data, kept, raw in cases.edge_pairs()}
    return {"inputs": inputs, "catalog": catalog, "edge_pairs": pairs}


def dump(v):
    """one line per block size, parameter set and pair; a SHA-256 that recurs (a stored block is the same at every ratio) is written once, in "sha256", and named by
    its index there"""
    shas = sorted({e[1] for section in ("inputs", "catalog") for group in v[section].values() for e in group.values()})
    index = {h: i for i, h in enumerate(shas)}
    packed = dict(v, sha256=shas, **{section: {k: {name: [e[0], index[e[1]]] for name, e in group.items()} for k, group in v[section].items()} for section in ("inputs", "catalog")})
    line = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))  # noqa: E731
    sections = ['"%s": {\n%s\n}' % (section, ",\n".join("%s: %s" % (json.dumps(k), line(packed[section][k])) for k in sorted(packed[section]))) for section in ("catalog", "edge_pairs", "inputs")]
    return "{\n%s,\n\"sha256\": [\n%s\n]\n}\n" % (",\n".join(sections), ",\n".join(", ".join(json.dumps(h) for h in shas[i:i + 4]) for i in range(0, len(shas), 4)))


def load(path=PATH):
    """the file as vectors() returns it: [length, SHA-256] per case"""
    packed = json.load(open(path))
    shas = packed.pop("sha256")
    for section in ("inputs", "catalog"):
        packed[section] = {k: {name: [e[0], shas[e[1]]] for name, e in group.items()} for k, group in packed[section].items()}
    return packed


if __name__ == "__main__":
    with open(PATH, "w") as f:
        f.write(dump(vectors()))
    print("wrote %s" % PATH)
