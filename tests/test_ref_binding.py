"""The drop-in boundary end to end: REAL reference fastp (its CLI, reader / writer threads, Stats / FilterResult
objects, JSON reporter) with the two worker-loop bodies bound to the engine by oracle/patches/gpu_worker.cpp
(oracle/build_ref_gpu.sh -> oracle/_ref/fastp_ref_gpu), against the unpatched reference `fastp_ref -w 1` on the same
files: every output FASTQ byte for byte, and the JSON report fastp ITSELF wrote, value for value.

The CPU suite runs the binding linked against the SIMT-emulator build of the engine (fastp_ref_gpusim, small
inputs); the `-m gpu` test runs the real library.  Both binaries are built in the build container (they need
/root/reference) and travel to the GPU box with oracle/_ref/."""
import json
import os
import sys
import subprocess

import pytest

import cases
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "fastp_ref")
REF_GPU = os.path.join(ROOT, "oracle", "_ref", "fastp_ref_gpu")
REF_SIM = os.path.join(ROOT, "oracle", "_ref", "fastp_ref_gpusim")

# case -> extra CLI flags that name the secondary outputs the case exercises
BINDING_CASES = {
    "pe_default": [],
    "pe_cut_right": [],
    "pe_cut_front_tail": [],
    "pe_polyg_polyx": [],
    "pe_adapter_seq": [],
    "pe_correction": [],
    "pe_trim_fixed": [],
    "pe_filters": ["--unpaired1", "@TMP@/u1.fq", "--unpaired2", "@TMP@/u2.fq"],
    "pe_noadapter_dedup": [],
    "pe_nofilters": [],
    "pe_merge": [],
    "pe_merge_unmerged": [],
    "pe_allow_gap_indel": [],
    "pe_umi_per_read": [],
    "pe_adapter_fasta": [],
    "pe_overrep": [],
    "pe_overlapped_out_trims": [],
    "pe_overlapped_out_noadapter": [],
    "pe_merge_overlapped_out_trims": [],
    # letters outside ACGTN (soft-masked stretches, IUPAC codes, '.'): the text kernel, through both bindings
    "pe_exotic_default": [],
    "pe_exotic_merge": [],
    "pe_exotic_dedup_adapters": [],
    "se_exotic_adapter": [],
    "pe_exotic_overrep_merge": [],   # -p as well: seeds may hold such letters, the counting kernel reads the units' text
    "se_exotic_overrep": [],
    "se_default_noadapter": [],
    "se_adapter_cut": [],
    "se_umi_read1": [],
    "se_adapter_indel": [],
    "se_overrep": [],
    "pe_adapter_long": [],
    "se_adapter_long_indel": [],
    "pe_late_long_reads": [],     # reads longer than the length the Evaluator saw in the first 1000: the stream re-plans
    "se_late_long_reads": [],
}


_BUILT = False


def _ensure_built():
    global _BUILT
    import engines
    if not _BUILT and os.path.isdir("/root/reference/src"):
        import __graft_entry__ as g
        engines.build_sim()     # the emulator build of the engine, which fastp_ref_gpusim links
        g.build()               # libfastp_gpu.so, fastp_ref, fastp_ref_gpu (+ fastp_ref_gpusim now that the emulator exists)
        subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref_gpu.sh")], stdout=subprocess.DEVNULL)
        _BUILT = True
    elif os.path.exists(REF_SIM):
        engines.build_sim()     # oracle/_ref/ was built in another tree: the emulator library it links is this tree's own
    return os.path.exists(REF)


def _run(binary, tmp, tag, flags, paired, gpu_env, threads=1, gz=False, in1=None, in2=None, interleaved=False, stdin_pipe=False):
    out = os.path.join(tmp, tag)
    os.makedirs(out, exist_ok=True)
    ext = ".fq.gz" if gz else ".fq"
    feed = None
    if stdin_pipe:      # --stdin: in1's bytes arrive through a pipe
        feed = open(in1 or os.path.join(tmp, "in1.fq"), "rb").read()
    cmd = [binary] + (["--stdin"] if stdin_pipe else ["-i", in1 or os.path.join(tmp, "in1.fq")]) + ["-o", os.path.join(out, "o1" + ext), "-j", os.path.join(out, "r.json"),
           "-h", os.path.join(out, "r.html"), "-w", str(threads), "--failed_out", os.path.join(out, "failed" + ext)]
    if paired and interleaved:      # both mates in in1
        cmd += ["--interleaved_in", "-O", os.path.join(out, "o2" + ext)]
    elif paired:
        cmd += ["-I", in2 or os.path.join(tmp, "in2.fq"), "-O", os.path.join(out, "o2" + ext)]
    cmd += [x.replace("@TMP@", out) for x in flags]
    env = dict(os.environ)
    env.pop("FASTP_GPU", None)
    env.update(gpu_env)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=1200, input=feed)
    assert p.returncode == 0, f"{os.path.basename(binary)} failed: {p.stderr.decode()[-1500:]}"
    files = {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out)) if fn.endswith(".fq")}
    for fn in sorted(os.listdir(out)):   # ".gz" outputs: concatenated gzip members, compared by what they inflate to
        if fn.endswith(".fq.gz"):
            import gzip
            files[fn] = gzip.decompress(open(os.path.join(out, fn), "rb").read())
    rep = json.load(open(os.path.join(out, "r.json")))
    rep.pop("command", None)
    rep["__stderr__"] = p.stderr.decode(errors="replace")
    return files, rep


def _diff(x, y, path, out):
    if isinstance(x, dict) and isinstance(y, dict):
        for k in sorted(set(x) | set(y)):
            if k not in x or k not in y:
                out.append(f"{path}/{k}: only on one side")
            else:
                _diff(x[k], y[k], f"{path}/{k}", out)
    elif isinstance(x, list) and isinstance(y, list):
        if len(x) != len(y):
            out.append(f"{path}: {len(x)} vs {len(y)} entries")
        else:
            for i, (p, q) in enumerate(zip(x, y)):
                _diff(p, q, f"{path}[{i}]", out)
    elif x != y:
        out.append(f"{path}: reference {x!r} binding {y!r}")


# the emulator runs a launch per kernel lane by lane: small chunks keep its parser launches short AND make every run
# take several trips (carried partial records, the mates' different record sizes)
SIM_ENV = {"FASTP_GPU_STREAM_CHUNK_BYTES": "70000"}
PACK_MODE = {"FASTP_GPU_STREAM": "0"}   # the reference's own reader threads + the worker-loop hooks


def _check(name, binary, n, tmp_path, seed, threads=1, extra_env=None, eol=b"\n", trailing=True, gz=False, more_flags=(),
           mode="stream", mutate=None, expect_units=None, gz_in=None, interleaved=False, stdin_pipe=False, ref_on_phred33=False):
    """ref_on_phred33: the REFERENCE run gets the same records with their qualities already converted (max(33, q - 31)) and no
    --phred64 - what --phred64 means.  The reference's own --phred64 converts in Read's constructor only
    (fastqreader.cpp:364-367): a Read object that comes back from its ReadPool keeps the file's characters, so once the pool
    has objects to hand out (after the first pack of 1000 has been processed - a matter of thread timing) its output is a
    mixture of converted and unconverted reads.  Direct comparisons with `fastp_ref --phred64` therefore use inputs of one pack."""
    paired, flags, pf, skw = cases.CASES[name]
    flags = list(flags) + BINDING_CASES[name] + list(more_flags)
    tmp = str(tmp_path)
    d = synth.synth_pairs(n, L=150, seed=seed, paired=paired, **skw)
    if mutate:
        mutate(d)

    def text(seq, qual, lens, mate):   # line ends as the caller wants them (FastqReader::getLine takes \n, \r\n and \r)
        t = synth.to_fastq(seq, qual, lens, mate).replace(b"\n", eol)
        return t if trailing else t[:len(t) - len(eol)]
    with open(os.path.join(tmp, "in1.fq"), "wb") as f:
        f.write(text(d["seq1"], d["qual1"], d["len1"], 1))
    if paired:
        with open(os.path.join(tmp, "in2.fq"), "wb") as f:
            f.write(text(d["seq2"], d["qual2"], d["len2"], 2))
    for fn, content in cases.FILES.get(name, {}).items():
        for tag in ("ref", "gpu"):
            os.makedirs(os.path.join(tmp, tag), exist_ok=True)
            with open(os.path.join(tmp, tag, fn), "wb") as f:
                f.write(content)
    if interleaved:   # --interleaved_in: the two files dealt into one (read 1, read 2, read 1, ...), which takes in1.fq's place
        a = open(os.path.join(tmp, "in1.fq"), "rb").read().split(eol)
        b = open(os.path.join(tmp, "in2.fq"), "rb").read().split(eol)
        recs = []
        for i in range(0, min(len(a), len(b)) - 3, 4):
            recs += a[i:i + 4] + b[i:i + 4]
        with open(os.path.join(tmp, "in1.fq"), "wb") as f:
            f.write(eol.join(recs) + (eol if trailing else b""))
        os.remove(os.path.join(tmp, "in2.fq"))
    in1 = in2 = None
    if gz_in:   # ".gz" inputs, read by BOTH binaries (the reference here inflates through oracle/shims/isa-l over zlib)
        in1, in2 = _compress_inputs(tmp, paired, gz_in)
    ref_flags, ref_in1, ref_in2, ref_tmp = flags, in1, in2, tmp
    if ref_on_phred33:
        assert "--phred64" in flags
        ref_flags = [f for f in flags if f != "--phred64"]
        ref_tmp = os.path.join(tmp, "ref33")
        os.makedirs(ref_tmp, exist_ok=True)
        for fn in ("in1.fq", "in2.fq"):
            if not os.path.exists(os.path.join(tmp, fn)):
                continue
            lines = open(os.path.join(tmp, fn), "rb").read().split(eol)
            for i in range(3, len(lines), 4):
                lines[i] = bytes(max(33, c - 31) for c in lines[i])
            with open(os.path.join(ref_tmp, fn), "wb") as f:
                f.write(eol.join(lines))
        ref_in1 = ref_in2 = None
        if gz_in:
            ref_in1, ref_in2 = _compress_inputs(ref_tmp, paired, gz_in)
        for fn, content in cases.FILES.get(name, {}).items():
            os.makedirs(os.path.join(ref_tmp, "ref"), exist_ok=True)
            with open(os.path.join(ref_tmp, "ref", fn), "wb") as f:
                f.write(content)
    want_files, want_rep = _run(REF, ref_tmp, "ref", ref_flags, paired, {}, gz=gz, in1=ref_in1, in2=ref_in2, interleaved=interleaved, stdin_pipe=stdin_pipe)
    env = {"FASTP_GPU": "1", "FASTP_GPU_VERBOSE": "1"}
    if binary == REF_SIM:
        env.update(SIM_ENV)
    if mode == "pack":
        env.update(PACK_MODE)
    env.update(extra_env or {})
    got_files, got_rep = _run(binary, tmp, "gpu", flags, paired, env, threads=threads, gz=gz, in1=in1, in2=in2, interleaved=interleaved, stdin_pipe=stdin_pipe)
    err = got_rep.pop("__stderr__")
    want_rep.pop("__stderr__")
    # which binding ran: the stream loop says so
    streamed = "fastp_gpu: stream mode:" in err
    assert streamed == (mode == "stream"), err[-800:]
    if "overrep" in name and "exotic" not in name:   # -p: the Evaluator's substring census ran on the device too (fastp_gpu_eval_overrep;
        # a sample with letters outside ACGTN is left to the reference's own Evaluator)
        # (with --interleaved_in the reference itself calls computeOverRepSeq ONCE: in2 is empty, evaluator.cpp:171-176)
        assert err.count("computeOverRepSeq on the device") == (2 if (paired and not interleaved) else 1), err[-800:]
        if n >= 10000:   # (600 reads do not reach the count thresholds: both sides then agree on "none")
            assert len(want_rep["read1_before_filtering"]["overrepresented_sequences"]) > 0
    assert sorted(want_files) == sorted(got_files)
    for fn in want_files:
        assert want_files[fn] == got_files[fn], f"{name}: {fn} differs ({len(want_files[fn])} vs {len(got_files[fn])} bytes)"
    problems = []
    _diff(want_rep, got_rep, "", problems)
    assert not problems, f"{name}: fastp's own JSON report differs:\n" + "\n".join(problems[:25])
    assert want_rep["summary"]["before_filtering"]["total_reads"] == (2 if paired else 1) * (n if expect_units is None else expect_units)
    return err


IL_BINDING_CASES = [("pe_default", dict(threads=2)), ("pe_merge_unmerged", dict(threads=1, eol=b"\r\n")),
                    ("pe_exotic_dedup_adapters", dict(threads=3, gz_in=("bgzf",), gz=True)), ("pe_overrep", dict(threads=4, gz_in=("members",)))]


# (every `-m gpu` parametrisation of tests/test_zz_gpu_compressed_inputs.py runs here on the emulator first: the lists are shared and
# tests/conftest.py refuses a collection in which a GPU case has no emulator twin)
@pytest.mark.parametrize("name,kw", IL_BINDING_CASES +
                                    [("pe_merge_unmerged", dict(threads=1, eol=b"\r\n", more_flags=("--reads_to_process", "500"), expect_units=500)),
                                     ("pe_correction", dict(threads=2, mode="pack", extra_env={"FASTP_GPU_STREAM_INTERLEAVED": "0"}))])
def test_patched_reference_interleaved_input(name, kw, tmp_path):
    """--interleaved_in (PairEndProcessor::interleavedReaderTask): the stream deals the one file's records out to the mates on the
    device; FASTP_GPU_STREAM_INTERLEAVED=0 keeps the reference's own interleaved reader (pack mode)"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 700, tmp_path, seed=58, interleaved=True, **kw)


STDIN_CASES = [("se_adapter_cut", dict(threads=2)), ("pe_filters", dict(threads=3, interleaved=True)), ("se_default_noadapter", dict(threads=1, eol=b"\r\n", gz=True)),
               ("pe_merge_unmerged", dict(threads=2, interleaved=True, more_flags=("--reads_to_process", "400"), expect_units=400))]


@pytest.mark.parametrize("name,kw", STDIN_CASES)
def test_patched_reference_stdin_input(name, kw, tmp_path):
    """--stdin (in1 = "/dev/stdin", a pipe; with --interleaved_in for paired data): the stream reads the pipe in sequence into
    its page-locked slots; the Evaluator does not run on such input in the reference (main.cpp:437), so the evaluated read
    length is the default and longer reads re-plan"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 700, tmp_path, seed=60, stdin_pipe=True, **kw)


def _to_phred64(d):
    """the synthetic reads' qualities moved to the phred+64 scale (with a few below '@', which convertPhred64To33 clamps to '!')"""
    import numpy as np
    rng = np.random.default_rng(9)
    for m in ("1", "2"):
        q = d.get("qual" + m)
        if q is None:
            continue
        body = q >= 33
        q[body] = np.minimum(q[body] + 31, 126)
        low = body & (rng.random(q.shape) < 0.01)
        q[low] = rng.integers(59, 64, size=int(low.sum())).astype(q.dtype)


PHRED64_CASES = [("pe_default", dict(threads=2)), ("se_adapter_cut", dict(threads=3, eol=b"\r\n")), ("pe_exotic_merge", dict(threads=1, gz_in=("bgzf", "gzip"))),
                 ("pe_filters", dict(threads=2, interleaved=True)), ("se_overrep", dict(threads=2, gz=True))]


@pytest.mark.parametrize("name,kw", PHRED64_CASES +
                         [("pe_correction", dict(threads=2, mode="pack", extra_env={"FASTP_GPU_STREAM": "0"}))])
def test_patched_reference_phred64_input(name, kw, tmp_path):
    """--phred64: FastqReader::read converts every read's qualities (Read::convertPhred64To33); the stream does it on the device
    right after the parser (fastp_gpu_phred64_to_33: the text the formatter prints and the packed rows), pack mode gets
    converted reads from the reference's reader"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 700, tmp_path, seed=59, mutate=_to_phred64, more_flags=("--phred64",), **kw)   # one pack: the reference converts every read
    if kw.get("mode") != "pack":   # several packs against what --phred64 means (pack mode takes the reference's own reads: its mixture)
        sub = tmp_path / "twin"
        sub.mkdir()
        _check(name, REF_SIM, 3000, sub, seed=61, mutate=_to_phred64, more_flags=("--phred64",), ref_on_phred33=True, **kw)


def _compress_inputs(tmp, paired, how):
    """in1.fq / in2.fq -> .fq.gz: "bgzf" = bgzip's members (9000 bytes of text each here: many per trip), "gzip" = one member,
    "members" = a few plain gzip members one behind the other"""
    import gzip
    import bgzf_util
    paths = []
    for k, h in zip((1, 2) if paired and len(how) > 1 else (1,), how):
        text = open(os.path.join(tmp, f"in{k}.fq"), "rb").read()
        if h == "bgzf":
            blob = bgzf_util.compress(text, block_bytes=9000)
        elif h == "gzip":
            blob = gzip.compress(text, 5)
        else:
            # (member ends become buffer ends in the reference's reader, and its line splitter loses the '\n' of a "\r\n" that
            # straddles or ends a buffer - fastqreader.cpp:257-259 `end < mBufDataLen-1` - and then stops at a bogus malformed
            # record; the stream parses the text itself and reads on, DESIGN.md 1.  Not what this test is about: cut elsewhere)
            def cut_at(c):
                while text[c - 1:c] == b"\r" or text[c - 2:c] == b"\r\n":
                    c += 1
                return c
            a, b = cut_at(len(text) // 3), cut_at(2 * (len(text) // 3) + 7)
            blob = gzip.compress(text[:a], 1) + gzip.compress(text[a:b], 9) + gzip.compress(text[b:], 4)
        paths.append(os.path.join(tmp, f"in{k}.fq.gz"))
        open(paths[-1], "wb").write(blob)
    return paths[0], (paths[1] if len(paths) > 1 else None)


# on the emulator (CPU suite) every flag set the real library sees in test_gpu_patched_reference_equals_reference (the twin rule of
# tests/conftest.py), at 600 units
EMULATOR_CASES = list(BINDING_CASES)
assert all(n in BINDING_CASES for n in EMULATOR_CASES)


def _overlapped_out(name):
    return any("overlapped_out" in f for f in cases.CASES[name][1])


@pytest.mark.parametrize("name", EMULATOR_CASES)
def test_patched_reference_on_emulator_equals_reference(name, tmp_path):
    """stream mode (the default): raw chunks -> device parser -> worker loop -> device formatter -> the writers' files"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    err = _check(name, REF_SIM, 600, tmp_path, seed=41)
    import re
    m = re.search(r"stream mode: 600 units in (\d+) chunks", err)
    assert m and int(m.group(1)) >= 2, err[-600:]    # several trips, so partial records were carried


@pytest.mark.parametrize("name", ["pe_correction", "pe_adapter_fasta", "pe_merge", "se_umi_read1", "pe_exotic_dedup_adapters", "se_exotic_adapter",
                                  "pe_overlapped_out_trims"])
def test_patched_reference_pack_mode_on_emulator(name, tmp_path):
    """pack mode: the reference's own reader threads, the hook at the top of the worker-loop body"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 600, tmp_path, seed=41, mode="pack")


@pytest.mark.parametrize("name,threads,writer", [("pe_filters", 2, "input"), ("se_adapter_cut", 4, "input"), ("pe_merge_unmerged", 5, None)])
def test_patched_reference_stream_threads_and_writer_handoff(name, threads, writer, tmp_path):
    """the stream's result does not depend on -w; FASTP_GPU_WRITER=input hands the text to WriterThread::input (one string
    per chunk, the threads' lists in turn) instead of writing into the writers' file descriptors"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 900, tmp_path, seed=52, threads=threads, extra_env={"FASTP_GPU_WRITER": writer} if writer else None)


@pytest.mark.parametrize("name,threads,writer", [("pe_default", 1, None), ("pe_default", 3, None), ("pe_filters", 3, "input")])
def test_patched_reference_stream_gz_outputs(name, threads, writer, tmp_path):
    """".gz" outputs: gzip members made on the device (fastp_gpu_deflate_bgzf) written into the WriterThread's file - its
    pwrite mode with several threads, its Writer with one - and bgzip's end-of-file member; or (writer = input) text
    compressed by the reference itself.  Compared by content."""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 700, tmp_path, seed=53, threads=threads, gz=True, extra_env={"FASTP_GPU_WRITER": writer} if writer else None)


GZ_BINDING_CASES = [("pe_default", ("bgzf", "bgzf"), dict(threads=4)), ("pe_overrep", ("bgzf", "gzip"), dict(threads=4)),
                    ("se_adapter_cut", ("bgzf",), dict(threads=4)), ("se_default_noadapter", ("members",), dict(threads=4))]   # (also the -m gpu list)


@pytest.mark.parametrize("name,how,kw", GZ_BINDING_CASES +
                                        [("se_adapter_cut", ("bgzf",), dict(threads=3, gz=True)),
                                         ("pe_exotic_dedup_adapters", ("members", "bgzf"), dict(threads=2, more_flags=("--reads_to_process", "500"), expect_units=500)),
                                         ("pe_correction", ("bgzf", "gzip"), dict(threads=2, mode="pack", extra_env={"FASTP_GPU_STREAM_GZ": "0"}))])
def test_patched_reference_compressed_inputs(name, how, kw, tmp_path):
    """".gz" inputs: bgzip-written files go to the device compressed and are inflated there (in place of BgzfMtReader), other
    gzip streams are inflated by zlib inside the stream; FASTP_GPU_STREAM_GZ=0 leaves them to the reference's reader (pack mode).
    Both binaries read the same compressed files."""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    err = _check(name, REF_SIM, 700, tmp_path, seed=57, gz_in=how, **kw)
    if kw.get("mode") != "pack":
        assert ("inflated on the device" in err) == ("bgzf" in how), err[-800:]


@pytest.mark.parametrize("mode", ["stream", "pack"])
@pytest.mark.parametrize("name,n,limit,threads", [("pe_default", 3000, 1500, 2), ("pe_default", 3000, 1000, 2), ("se_adapter_cut", 2500, 2000, 4)])
def test_patched_reference_reads_to_process(name, n, limit, threads, mode, tmp_path):
    """--reads_to_process: the reader stops after N reads (a short pack followed by an empty one in pack mode,
    a record cap on the trips in stream mode)"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, n, tmp_path, seed=54, threads=threads, more_flags=["--reads_to_process", str(limit)], mode=mode, expect_units=limit)


@pytest.mark.parametrize("mode", ["stream", "pack"])
@pytest.mark.parametrize("name,n,threads", [("pe_default", 3000, 4), ("se_default_noadapter", 3000, 4)])
def test_patched_reference_read_count_multiple_of_pack_size(name, n, threads, mode, tmp_path):
    """reads % 1000 == 0: the reader ends the stream with an EMPTY pack, which can be a worker's first pack"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, n, tmp_path, seed=55, threads=threads, mode=mode)


def _lengthen_late_reads(d):
    """reads longer than anything among the first 1000 (what Evaluator::computeSeqLen looks at)"""
    import numpy as np
    for m in ("1", "2"):
        if "seq" + m not in d or d["seq" + m] is None:
            continue
        seq, qual, lens = d["seq" + m], d["qual" + m], d["len" + m]
        lens[:1200] = np.minimum(lens[:1200], 100)
        assert lens[1200:].max() > 100


@pytest.mark.parametrize("name", ["se_adapter_cut", "pe_noadapter_dedup"])   # (with -p: tests/test_stream_abi.py, golden se_late_long_reads)
def test_patched_reference_stream_replans_for_longer_reads(name, tmp_path):
    """the first 1000 reads are at most 100 bases, later ones 150: the reference sizes its buffers from the first 1000 and
    grows them (Stats::extendBuffer); the stream re-plans - counters, Duplicate's bitmaps and the sampling positions of
    the overrepresentation analysis carried into a context with a larger max_len - and the report is the same"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    err = _check(name, REF_SIM, 2600, tmp_path, seed=56, mutate=_lengthen_late_reads)
    import re
    m = re.search(r"max_len (\d+), (\d+) re-plan", err)
    assert m and int(m.group(2)) >= 1 and int(m.group(1)) >= 150, err[-600:]


def _auto_adapter_check(binary, n, tmp_path):
    """SE run with adapter auto-detection on reads that carry an adapter fastp does not know (so checkKnownAdapters does
    not short-cut the k-mer path): the Evaluator's ten-mer histogram (evaluator.cpp:384-396) comes from
    fastp_gpu_eval_adapter_kmers; it is compared bin by bin with the reference's own counting loop inside the binding
    (FASTP_GPU_EVAL_CHECK), and the whole run that follows must equal the unpatched reference's"""
    tmp = str(tmp_path)
    custom = b"CTGACCTAGTCAAGGTCCATGCTAGGATCCATGCAAT"
    old = synth.ADAPTER_R1
    synth.ADAPTER_R1 = custom
    try:
        d = synth.synth_pairs(n, L=150, seed=47, paired=False, insert_mean=110.0, insert_sd=25.0, dup_frac=0.0)
    finally:
        synth.ADAPTER_R1 = old
    with open(os.path.join(tmp, "in1.fq"), "wb") as f:
        f.write(synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1))
    flags = ["-G"]
    want_files, want_rep = _run(REF, tmp, "ref", flags, False, {})
    got_files, got_rep = _run(binary, tmp, "gpu", flags, False, {"FASTP_GPU": "1", "FASTP_GPU_VERBOSE": "1", "FASTP_GPU_EVAL_CHECK": "1"})
    err = got_rep.pop("__stderr__")
    want_rep.pop("__stderr__")
    assert "ten-mer histogram on the device" in err, err[-600:]
    # FASTP_GPU_EVAL_CHECK: the binding also ran the reference's own counting loop (Evaluator::seq2int) and compared all 4^10 bins
    import re
    m = re.search(r"ten-mer histogram check vs Evaluator::seq2int: (\d+) of 1048576 bins differ \((\d+) non-zero\)", err)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) > 1000, err[-600:]
    for fn in want_files:
        assert want_files[fn] == got_files[fn], f"{fn} differs"
    problems = []
    _diff(want_rep, got_rep, "", problems)
    assert not problems, "fastp's own JSON report differs:\n" + "\n".join(problems[:25])


def test_patched_reference_auto_adapter_on_emulator(tmp_path):
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _auto_adapter_check(REF_SIM, 11000, tmp_path)


@pytest.mark.gpu
def test_gpu_patched_reference_auto_adapter(tmp_path):
    if not (os.path.exists(REF) and os.path.exists(REF_GPU)):
        pytest.skip("oracle/_ref binaries did not travel to this box")
    _auto_adapter_check(REF_GPU, 60000, tmp_path)


@pytest.mark.parametrize("name,threads,packs", [("pe_default", 3, 2), ("se_default_noadapter", 2, 1)])
def test_patched_reference_pipelines_windows_of_packs(name, threads, packs, tmp_path):
    """several worker threads, windows of FASTP_GPU_PACKS packs, more windows than slots in flight: the binding packs
    the threads' packs into windows in STREAM order, so the outputs and the whole report equal `fastp_ref -w 1`
    whatever the thread count (duplicates and insert sizes included)"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 9300, tmp_path, seed=43, threads=threads, extra_env={"FASTP_GPU_PACKS": str(packs)}, mode="pack")


@pytest.mark.parametrize("eol,trailing,mode", [(b"\r\n", True, "stream"), (b"\r", True, "stream"), (b"\n", False, "stream"), (b"\r\n", False, "stream"),
                                               (b"\r\n", True, "pack"), (b"\r", False, "pack")])
def test_patched_reference_reader_hook_line_ends(eol, trailing, mode, tmp_path):
    """the memchr hook in front of FastqReader::getLine's scan (fastp_gpu_reader_scan_eol): the same records from \\r\\n, \\r
    and unterminated last lines as the reference's own character-by-character scan (whose binary runs without the hook)"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check("pe_cut_right", REF_SIM, 2300, tmp_path, seed=47, threads=2, eol=eol, trailing=trailing, mode=mode)


def test_patched_reference_reader_hook_across_buffer_refills(tmp_path):
    """input files larger than FastqReader's 8 MiB buffer: lines that straddle a refill take getLine's second scan"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check("se_default_noadapter", REF_SIM, 52000, tmp_path, seed=48, threads=2, eol=b"\r\n", mode="pack")


@pytest.mark.parametrize("name,kw", [("pe_exotic_merge", dict(eol=b"\r\n", threads=3)), ("se_exotic_adapter", dict(gz=True, threads=4)),
                                     ("pe_exotic_dedup_adapters", dict(gz=True, threads=2, mode="pack")),
                                     ("se_exotic_overrep", dict(eol=b"\r", trailing=False, threads=2, more_flags=("--reads_to_process", "700"),
                                                                expect_units=700))])
def test_patched_reference_exotic_letters_with_line_ends_gz_and_limits(name, kw, tmp_path):
    """letters outside ACGTN together with what else the stream has to get right: other line ends, several -w, ".gz" outputs,
    --reads_to_process, pack mode"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    _check(name, REF_SIM, 1500, tmp_path, seed=11, **kw)


def test_patched_reference_exotic_letters_in_reads_longer_than_evaluated(tmp_path):
    """the stream re-plans for a longer read while units with letters outside ACGTN (and -p) are in flight"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    paired, flags, pf, skw = cases.CASES["se_late_long_reads"]
    cases.CASES["_se_late_long_exotic"] = (False, flags, pf, dict(skw, exotic_frac=0.1))
    BINDING_CASES["_se_late_long_exotic"] = []
    try:
        err = _check("_se_late_long_exotic", REF_SIM, 1700, tmp_path, seed=5)
        assert "1 re-plan(s)" in err, err[-400:]
    finally:
        del cases.CASES["_se_late_long_exotic"], BINDING_CASES["_se_late_long_exotic"]


@pytest.mark.parametrize("seed", range(2000, 2006))
def test_patched_reference_random_command_lines(seed):
    """tools/binding_fuzz.py: a random fastp command line on a random input (line ends, -w, ".gz", stream or pack binding, letters
    outside ACGTN) - every output file and the JSON report equal to the reference's (1000 more: profiles/r04_binding_fuzz_emulator.txt)"""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import binding_fuzz
    problems, c = binding_fuzz.run(seed, REF_SIM, True)
    assert not problems, f"{' '.join(c['flags'])} [{c['mode']}, -w {c['threads']}]: " + "; ".join(problems[:6])


@pytest.mark.gpu
@pytest.mark.twin("test_patched_reference_on_emulator_equals_reference")
@pytest.mark.parametrize("name", list(BINDING_CASES))
def test_gpu_patched_reference_equals_reference(name, tmp_path):
    """the same on the real library: fastp_ref_gpu (FASTP_GPU=1) vs fastp_ref, 30 000 units"""
    if not (os.path.exists(REF) and os.path.exists(REF_GPU)):
        pytest.skip("oracle/_ref binaries did not travel to this box")
    if _overlapped_out(name):   # the binding this test has always run for them; their stream-mode runs are in tests/test_zz_gpu_compressed_inputs.py
        _check(name, REF_GPU, 30000, tmp_path, seed=43, mode="pack", extra_env={"FASTP_GPU_STREAM_OVERLAPPED": "0"})
        return
    _check(name, REF_GPU, 30000, tmp_path, seed=43)


def test_patched_reference_pack_mode_with_a_lagging_read1_reader(tmp_path):
    """read 1's reader thread is slowed down (an LD_PRELOAD shim delays every fread on in1.fq, tests/slowread): a worker's
    loop then ends on its exhausted read-2 list while the read-1 reader is still producing packs for other workers
    (processorTask's second exit).  The stream's length must not be published from the read-1 counter at that moment
    (the last window was submitted short and its owners waited forever)."""
    if not _ensure_built() or not os.path.exists(REF_SIM):
        pytest.skip("reference binaries not built (no /root/reference here)")
    tmp = str(tmp_path)
    shim = os.path.join(tmp, "slowread.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "slowread", "slowread.c"), "-ldl", "-o", shim])
    n = 9300     # 10 packs per file; FastqReader fills 8 MiB at a time, so the file is a handful of freads
    d = synth.synth_pairs(n, L=150, seed=61, paired=True)
    with open(os.path.join(tmp, "in1.fq"), "wb") as f:
        f.write(synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1))
    with open(os.path.join(tmp, "in2.fq"), "wb") as f:
        f.write(synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2))
    want_files, want_rep = _run(REF, tmp, "ref", [], True, {})
    env = {"FASTP_GPU": "1", "FASTP_GPU_VERBOSE": "1", "FASTP_GPU_PACKS": "2", "LD_PRELOAD": shim,
           "SLOWREAD_PATH": os.path.realpath(os.path.join(tmp, "in1.fq")), "SLOWREAD_US": "1500000"}
    env.update(PACK_MODE)
    got_files, got_rep = _run(REF_SIM, tmp, "gpu", [], True, env, threads=4)
    err = got_rep.pop("__stderr__")
    want_rep.pop("__stderr__")
    assert "stream mode" not in err
    for fn in want_files:
        assert want_files[fn] == got_files[fn], f"{fn} differs"
    problems = []
    _diff(want_rep, got_rep, "", problems)
    assert not problems, "\n".join(problems[:25])
