#!/usr/bin/env python3
"""Known answers of the reference's QuickLZ codec (quicklz.c compiled as it lies into oracle/_ref/libquicklz_ref.so, oracle/Makefile
`ref`) -> tests/golden/qlz_ref.json: what its qlz_decompress makes of the streams inside the shipped .clm caches (SHA-256), and the
length and SHA-256 of its qlz_compress output for every input of tests/test_mesh_cache.py's compressor comparison. Runs only where
oracle/_ref/ could be built:
    python tests/golden/make_qlz_golden.py
tests/test_mesh_cache.py checks the product's codec against these answers where the reference build is absent."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_mesh_cache as T  # noqa: E402


def main():
    R = C.CDLL(T.REF_SO)
    R.qlz_get_setting.restype = C.c_int
    R.qlz_compress.restype = C.c_size_t
    R.qlz_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    compress = []
    for raw in T.compressor_inputs():
        comp = C.create_string_buffer(len(raw) + 400)
        n = R.qlz_compress(raw, comp, len(raw), C.create_string_buffer(R.qlz_get_setting(1)))
        compress.append({"raw_len": len(raw), "comp_len": int(n), "sha256": hashlib.sha256(comp.raw[:n]).hexdigest()})
    caches = {rel: {"decoded_sha256": T.ref_decoded_sha256(rel)} for rel in T.FIXTURE_CLMS}
    with open(os.path.join(HERE, "qlz_ref.json"), "w") as f:
        json.dump({"caches": caches, "compress": compress}, f, indent=1)
    print(f"{len(compress)} compressor answers, {len(caches)} caches")


if __name__ == "__main__":
    main()
