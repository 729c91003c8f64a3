#!/usr/bin/env python3
"""Record the fixtures of tests/test_text_edges.py from the REAL reference binary (oracle/_ref/fastp_ref, built by
oracle/build_ref.sh), -w 1.  Inputs: the hand-built families of tests/text_util.py, nothing else.

    python tests/golden/text_edges/make_fixtures.py [family ...]

<family>.npz   the input FASTQ text, the flags, md5 + size of every FASTQ the reference wrote, its JSON report without "command"
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

import driver  # noqa: E402
import text_util as tu  # noqa: E402


def main():
    for name in sys.argv[1:] or tu.FAMILIES:
        fam = tu.family(name)
        fq1, fq2 = tu.fastq(fam)
        ref = driver.run_reference(fam.flags, fq1, fq2, extra_files=fam.files)
        rec = {"fq1": np.frombuffer(fq1, dtype=np.uint8)}
        if fq2 is not None:
            rec["fq2"] = np.frombuffer(fq2, dtype=np.uint8)
        meta = {"flags": fam.flags, "outputs": {}, "json": ref["json"]}
        for k in ("out1", "out2", "failed", "merged", "overlapped"):
            if ref.get(k) is not None:
                meta["outputs"][k] = {"md5": hashlib.md5(ref[k]).hexdigest(), "size": len(ref[k])}
        rec["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, {k: v["size"] for k, v in meta["outputs"].items()})


if __name__ == "__main__":
    main()
