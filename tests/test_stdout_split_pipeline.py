"""FastqPipeline.run(interleaved_out=..., split=...): --stdout's interleaved stream and --split's files through
fastp_amd/pipeline.py, against what the real reference wrote (tests/golden/output_files/).  The pipeline runs on torch tensors
of a GPU, so these are `-m gpu` tests only; the file loop's emulator cases (tests/test_stdout_split_stream.py) are their twins:
the pipeline makes the same calls (pack table, segment deflate) and follows the same rules."""
import os

import numpy as np
import pytest

import cases
import outfiles_util as ofu
from test_stdout_split_stream import GEOMETRIES, _chunk_bytes
from test_stream_abi import _files


def _umi(name):
    return cases.UMI.get(ofu.CASES[name]["base"])


def _run(pipe, name, p1, p2, out, **kw):
    """the case's run() call; returns the name of the file that holds the reference's standard output, if any"""
    c = ofu.CASES[name]
    paired = p2 is not None
    if c.get("split"):
        how, v = c["split"]
        ext = ".fq.gz" if c.get("gz") else ".fq"
        split = ("lines", v) if how == "lines" else ("files", v, ofu.reads_per_file(name))
        pipe.run(p1, p2, os.path.join(out, "o1" + ext), os.path.join(out, "o2" + ext) if paired else None, umi=_umi(name), split=split,
                 split_digits=c.get("digits", 4), **kw)
        return None
    extra = {("failed_out" if k == "failed" else k): os.path.join(out, k + ".fq") for k in c.get("want", ())}
    if pipe.params.merge:    # --merge --stdout: the merged stream is what goes to standard output
        side = os.path.join(os.path.dirname(out), "side")
        os.makedirs(side, exist_ok=True)
        pipe.run(p1, p2, os.path.join(side, "o1.fq"), os.path.join(side, "o2.fq"), merged_out=os.path.join(out, "merged.fq"), umi=_umi(name), **kw)
        return "merged.fq"
    pipe.run(p1, p2, os.path.join(out, "out1.fq"), None, umi=_umi(name), interleaved_out=paired, **extra, **kw)
    return "out1.fq"


def _pipeline_case(name, geometry, tmp_path):
    from fastp_amd.pipeline import FastqPipeline
    fq1, fq2, meta = ofu.load(name)
    params = ofu.case_params(name)
    p1, p2 = _files(tmp_path, fq1, fq2)
    out = str(tmp_path / "run")
    os.mkdir(out)
    pipe = FastqPipeline(params, device=0, chunk_bytes=_chunk_bytes(geometry, fq1, fq2))
    try:
        main = _run(pipe, name, p1, p2, out)
        stats = dict(pipe.stats)
        ctr = pipe.counters().copy()
    finally:
        pipe.close()
    expected = dict(meta["files"])
    if main:
        expected[main] = meta["stdout"]
    got = {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}
    assert sorted(got) == sorted(expected), (sorted(got), sorted(expected))
    for fn, exp in expected.items():
        text = ofu.text_of(fn, got[fn])
        assert (ofu.md5(text), len(text)) == (exp["md5"], exp["size"]), f"{name} {geometry}: {fn} differs from the reference's"
        assert not fn.endswith(".gz") or got[fn].endswith(ofu.BGZF_EOF)
    if ofu.CASES[name].get("split"):
        assert stats["split_files"] == len([fn for fn in got if fn.split(".")[1] == "o1"])
        assert geometry == "one_chunk" or stats["chunks"] >= 2
    # the counters of the run without --split / --stdout
    plain = FastqPipeline(ofu.case_params(name), device=0, chunk_bytes=1 << 22)
    try:
        d = str(tmp_path / "plain")
        os.mkdir(d)
        plain.run(p1, p2, os.path.join(d, "a.fq"), os.path.join(d, "b.fq") if p2 else None, umi=_umi(name),
                  merged_out=os.path.join(d, "m.fq") if params.merge else None)
        assert np.array_equal(plain.counters(), ctr)
    finally:
        plain.close()


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_output_files_equal_reference_golden")
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", list(ofu.CASES))
def test_gpu_pipeline_output_files_equal_reference_golden(name, geometry, tmp_path):
    _pipeline_case(name, geometry, tmp_path)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_output_setters_refuse")
def test_gpu_pipeline_split_and_interleaved_rules(tmp_path):
    """the rules of fastp_gpu_stream_set_split / _set_interleaved_output, as PipelineError"""
    from fastp_amd.pipeline import FastqPipeline, PipelineError
    pe, se = "split_pe_files5", "split_se_files2"
    o = lambda k: str(tmp_path / k)
    for name, bad in ((pe, [dict(split=("files", 5, 640), failed_out=o("f.fq")), dict(split=("files", 5, 640), unpaired1=o("u.fq")),
                            dict(split=("files", 5, 640), unpaired2=o("u.fq")), dict(split=("files", 1, 640)), dict(split=("files", 1000, 640)),
                            dict(split=("files", 5, 0)), dict(split=("lines", 4001)), dict(split=("lines", 0)), dict(split=("packs", 5)),
                            dict(split=("files", 5)), dict(split=("files", 5, 640), split_digits=11), dict(split=("files", 5, 640), split_digits=-1),
                            dict(split=("files", 5, 640), interleaved_out=True, out2=None), dict(split=("files", 5, 640), out2=None),
                            dict(interleaved_out=True)]),                       # (out2 given with interleaved_out)
                      (se, [dict(interleaved_out=True), dict(split=("files", 2, 1150), out1=None)]),
                      ("stdout_pe_merge", [dict(split=("lines", 4000), merged_out=o("m.fq")), dict(split=("lines", 4000)),
                                           dict(interleaved_out=True, out2=None, merged_out=o("m.fq"))])):
        fq1, fq2, _ = ofu.load(name)
        d = tmp_path / name
        d.mkdir()
        p1, p2 = _files(d, fq1, fq2)
        pipe = FastqPipeline(ofu.case_params(name), device=0, chunk_bytes=1 << 20)
        try:
            for kw in bad:
                kw = dict(kw)
                out1 = kw.pop("out1", o("o1.fq"))
                out2 = kw.pop("out2", o("o2.fq") if p2 else None)
                with pytest.raises(PipelineError):
                    pipe.run(p1, p2, out1, out2, **kw)
        finally:
            pipe.close()
