#!/usr/bin/env python3
"""Record the fixtures of tests/test_read_names.py from the REAL reference binary (oracle/_ref/fastp_ref, built by
oracle/build_ref.sh), -w 1.  Inputs: the name zoo and the parameter sets of tests/read_names_util.py, nothing else.

    python tests/golden/read_names/make_fixtures.py

names_table.json   the names the reference writes for every pair of the zoo (-A -G -Q -L: every read is written as it
                   came), for {index1, index2, per_index} x {--fix_mgi_id on, off} x {no prefix, prefix U and delimiter
                   "#~"}, paired and single-end (the reference's command line refuses index2 on single-end input)
<set>.npz          per parameter set of read_names_util.FILE_SETS: the input text (zoo-named synthetic reads), md5 + size of
                   every FASTQ the reference wrote, its JSON report, and the report of the same run WITHOUT the name options
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
import read_names_util as rn  # noqa: E402

PREFIXES = [("", ":"), ("U", "#~")]


def names_of(text):
    return [x.decode("latin-1") for x in text.split(b"\n")[0::4][:-1]]


def table():
    body = b"\nACGTACGTAC\n+\nIIIIIIIIII\n"
    fq1 = b"".join(a + body for a, _ in rn.ZOO)
    fq2 = b"".join(b + body for _, b in rn.ZOO)
    runs = []
    for paired in (True, False):
        for loc in rn.LOCATIONS:
            if loc == "index2" and not paired:
                continue
            for mgi in (False, True):
                for prefix, delim in PREFIXES:
                    flags = ["-A", "-G", "-Q", "-L", "-U", "--umi_loc", loc, "--umi_delim", delim]
                    if prefix:
                        flags += ["--umi_prefix", prefix]
                    if mgi:
                        flags.append("--fix_mgi_id")
                    ref = driver.run_reference(flags, fq1, fq2 if paired else None, want_failed=False)
                    run = dict(loc=loc, mgi=mgi, prefix=prefix, delimiter=delim, paired=paired, names1=names_of(ref["out1"]),
                               names2=names_of(ref["out2"]) if paired else None)
                    assert len(run["names1"]) == len(rn.ZOO)
                    runs.append(run)
    zoo = [[a.decode("latin-1"), b.decode("latin-1")] for a, b in rn.ZOO]
    with open(os.path.join(HERE, "names_table.json"), "w") as f:
        json.dump({"zoo": zoo, "runs": runs}, f, indent=0)
    print("names_table.json:", len(runs), "runs of", len(zoo), "names")


def file_sets():
    for name in rn.FILE_SETS:
        paired, plain_flags, flags, fq1, fq2 = rn.file_set_inputs(name)
        ref = driver.run_reference(flags, fq1, fq2)
        plain = driver.run_reference(plain_flags, fq1, fq2)
        rec = {"fq1": np.frombuffer(fq1, dtype=np.uint8)}
        if paired:
            rec["fq2"] = np.frombuffer(fq2, dtype=np.uint8)
        meta = {"flags": flags, "outputs": {}, "json": ref["json"], "json_plain": plain["json"]}
        for k in ("out1", "out2", "failed", "merged"):
            if ref.get(k) is not None:
                meta["outputs"][k] = {"md5": hashlib.md5(ref[k]).hexdigest(), "size": len(ref[k])}
        rec["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, {k: v["size"] for k, v in meta["outputs"].items()}, "json unchanged by the name options:",
              ref["json"] == plain["json"])


if __name__ == "__main__":
    table()
    file_sets()
