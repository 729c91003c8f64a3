"""Regenerate tests/golden/output_files/*.npz: what the real reference (oracle/_ref/fastp_ref -w 1) writes for --stdout and
for --split / --split_by_lines.  Run in the build container:
    python tests/golden/make_golden_output_files.py
A fixture holds the input text and, per file the reference wrote, its name and the md5 and size of its text (the inflated
text for ".gz"); for --stdout the same for the captured standard output.  The cases are tests/outfiles_util.py's CASES."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import outfiles_util as ofu  # noqa: E402

FASTP_REF = os.path.join(ROOT, "oracle", "_ref", "fastp_ref")
OUT = os.path.join(HERE, "output_files")


def records(text):
    return text.count(b"\n") // 4


def one(name):
    c = ofu.CASES[name]
    paired, flags, _, _ = cases.CASES[c["base"]]
    flags = list(flags)
    drop = c.get("drop_flags", [])
    flags = [f for f in flags if f not in drop] + c.get("flags", [])
    fq1, fq2 = ofu.case_input(name)
    tmp = tempfile.mkdtemp(prefix="fastp_out_")
    out = os.path.join(tmp, "out")
    os.mkdir(out)
    with open(os.path.join(tmp, "in1.fq"), "wb") as f:
        f.write(fq1)
    cmd = [FASTP_REF, "-i", os.path.join(tmp, "in1.fq"), "-j", os.path.join(tmp, "r.json"), "-h", os.path.join(tmp, "r.html"), "-w", "1"]
    if paired:
        with open(os.path.join(tmp, "in2.fq"), "wb") as f:
            f.write(fq2)
        cmd += ["-I", os.path.join(tmp, "in2.fq")]
    ext = ".fq.gz" if c.get("gz") else ".fq"
    if c.get("split"):
        how, v = c["split"]
        cmd += ["-o", os.path.join(out, "o1" + ext)] + (["-O", os.path.join(out, "o2" + ext)] if paired else [])
        cmd += (["-S", str(v)] if how == "lines" else ["-s", str(v)]) + ["-d", str(c.get("digits", 4))]
    if c.get("stdout"):
        cmd += ["--stdout"]
        for k in c.get("want", ()):
            cmd += ["--" + ("failed_out" if k == "failed" else k), os.path.join(out, k + ".fq")]
    cmd += flags
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError(name + ": fastp_ref failed: " + p.stderr.decode()[-2000:])
    files = {}
    for fn in sorted(os.listdir(out)):
        text = ofu.text_of(fn, open(os.path.join(out, fn), "rb").read())
        files[fn] = {"md5": ofu.md5(text), "size": len(text), "records": records(text)}
    meta = {"case": name, "files": files, "units": c["n"]}
    if c.get("stdout"):
        meta["stdout"] = {"md5": ofu.md5(p.stdout), "size": len(p.stdout), "records": records(p.stdout)}
        assert meta["stdout"]["records"] >= 100, (name, meta["stdout"])
    if c.get("split"):
        # no test may pass vacuously: enough files, and in the by-lines cases a pack that did not pass whole
        how, v = c["split"]
        per_stream = [k for k in files if k.endswith("o1" + ext)]
        assert (how == "files" and len(per_stream) == v) or len(per_stream) >= 3, (name, sorted(files))
        meta["reads_per_file"] = ofu.reads_per_file(name)
        total = sum(files[k]["records"] for k in per_stream)
        if how == "lines" and c["base"] != "pe_nofilters":
            assert total < c["n"] - 50, (name, total)       # reads fail, so packs count fewer than their units
        meta["ends_in_empty_file"] = files[sorted(per_stream, key=lambda k: int(k.split(".")[0]))[-1]]["size"] == 0
    rec = {"fq1": np.frombuffer(fq1, dtype=np.uint8), "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    if fq2 is not None:
        rec["fq2"] = np.frombuffer(fq2, dtype=np.uint8)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 476 * 1024, (name, os.path.getsize(path))
    print(name, os.path.getsize(path), "bytes;", {k: (v["size"], v["records"]) for k, v in files.items()}, meta.get("stdout", ""))
    return meta


def main():
    metas = [one(name) for name in ofu.CASES]
    assert any(m.get("ends_in_empty_file") for m in metas), "no split case ends in an empty file"


if __name__ == "__main__":
    main()
