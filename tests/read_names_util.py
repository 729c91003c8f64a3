"""helpers of tests/test_read_names.py: the name options of the output side - UMIs taken from the index part of the name
(--umi_loc index1 / index2 / per_index) and --fix_mgi_id - through the device formatter, the host writers and the file loop.
Own mirrors of the option words: tests/cpphost.py, tests/streamlib.py and tests/format_util.py know read1 / read2 / per_read."""
import ctypes as C
import json
import os

import numpy as np

import cases
import cpphost
import driver
import format7_util as f7
import streamlib
import synth
from fastp_amd import abi, hostloop

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_names")
STREAMS = f7.STREAMS

# ---- the name zoo: (name of read 1, name of read 2); the smallest set at which each rule of Read::firstIndex / lastIndex /
# fixMGI and addUmiToName's first space can go wrong
_LONG_NAME = b"@" + b"L" * 70
_LONG_INDEX = b"ACGT" * 17 + b"+" + b"TTGA" * 17
_N200 = b"@" + b"n" * 150 + b":" + b"c" * 20
ZOO = [
    (b"@SIM:1:FC:1:1101:0:7 1:N:0:ATCG", b"@SIM:1:FC:1:1101:0:7 2:N:0:ATCG"),   # Illumina, single index
    (b"@a", b"@b"),                                                              # length 2
    (b"@a:b", b"@a:c"),                                                          # length 4: below firstIndex's minimum
    (b"@a:bc", b"@a+bc"),                                                        # length 5
    (b"@ab:cd", b"@ab:cd"),                                                      # length 6
    (b"@abcdefg", b"@abcdefg"),                                                  # no ':'
    (b"@abcd:x", b"@abcd+x"),                                                    # ':' / '+' only among the last two characters
    (b"@abcde:", b"@abcde+"),
    (b"@r 1:N:0:ACGT+TTGA", b"@r 2:N:0:ACGT+TTGA"),                              # dual index
    (b"@r 1:N:0:ACGT+TT+GA", b"@r 2:N:0:ACGT+TT+GA"),                            # two '+'
    (b"@r 1:N:0:ACGT+T", b"@r 2:N:0:ACGT+T"),                                    # '+' in the last two characters
    (b"@p+qqqq", b"@p+qqqq"),                                                    # '+' with no ':' to its left
    (b"@r 1:N:0:+:AC", b"@r 2:N:0:+:AC"),                                        # "+:" adjacent
    (b"@r 1:N:0::+AC", b"@r 2:N:0::+AC"),                                        # ":+" adjacent: an empty first index
    (b"@M1:22:ACGTAC+TTGACA", b"@M1:22:ACGTAC+TTGACA"),                          # no space at all
    (b"@V300:L1:C2:R3/1", b"@V300:L1:C2:R3/2"),                                  # MGI
    (b"@/1", b"@/2"),
    (b"@x1", b"@x2"),                                                            # ends in 1 / 2 without the '/'
    (b"@V3/1", b"@V3/2"),
    (b"@q:AAAA/1", b"@q:AAAA/2"),
    (b"@w x:AC+GT/1", b"@w x:AC+GT/2"),                                          # a space of its own in front of the MGI one
    (b"@r 1:N:0:ACGT+TTGA", b"@rr 2:N:0:ACGTAA+TTGACCA"),                        # mates whose names differ in length
    (b"@V300:L1:C2:R3/1", b"@V300:L1:C2:R3 2"),                                  # only one mate gets the MGI fix
    (_LONG_NAME + b" 1:N:0:ACGT", _LONG_NAME + b" 2:N:0:ACGT"),                   # a name of more than 64 bytes
    (b"@i 1:N:0:" + _LONG_INDEX, b"@i 2:N:0:" + _LONG_INDEX),                     # indexes of more than 64 bytes
    (_N200 + b"/1", _N200 + b"/2"),                                              # 200 bytes: ':' far from the end, MGI
    (_N200 + b"+" + b"g" * 27, _N200 + b"+" + b"g" * 27),                        # 200 bytes
]
assert len(ZOO[-1][0]) == 200

LOCATIONS = ("index1", "index2", "per_index")


def editor(loc, fix_mgi=False, prefix=b"", delimiter=b":", umi_len=0):
    if loc is None and not fix_mgi:
        return None
    return hostloop.UmiNameEditor(loc, umi_len, prefix, delimiter, fix_mgi=fix_mgi)


def option_word(ed):
    """FASTP_GPU_UMI_* | FASTP_GPU_NAME_FIX_MGI of an editor"""
    if ed is None:
        return 0
    return (abi.UMI_LOC[ed.loc] if ed.loc else 0) | (abi.NAME_FIX_MGI if ed.fix_mgi else 0)


def zoo_fastq(d, paired, rot=0, name_of=None):
    """synthetic reads (tests/synth.py arrays) under the zoo's names, cycled: unit i is called ZOO[(i + rot) % len(ZOO)]"""
    out = []
    for m in ((1, 2) if paired else (1,)):
        seq, qual, lens = d["seq%d" % m], d["qual%d" % m], d["len%d" % m]
        parts = []
        for i in range(len(lens)):
            L = int(lens[i])
            name = name_of(i, m) if name_of else ZOO[(i + rot) % len(ZOO)][m - 1]
            parts += [name, b"\n", seq[i, :L].tobytes(), b"\n+\n", qual[i, :L].tobytes(), b"\n"]
        out.append(b"".join(parts))
    return out[0], (out[1] if paired else None)


def inputs(case, n, rot=0, seed=77, **extra):
    """(params, fq1, fq2) of a parameter set of tests/cases.py on zoo-named reads"""
    paired, flags, pf, skw = cases.CASES[case]
    d = synth.synth_pairs(n, L=150, seed=seed, paired=paired, **skw)
    p = pf(150)
    for k, v in extra.items():
        setattr(p, k, v)
    fq1, fq2 = zoo_fastq(d, paired, rot)
    return p, fq1, fq2


def expected(mk_engine, params, fq1, fq2, max_len, want_failed, want_unpaired, ed, cpp_lib=None):
    """{stream: bytes} of the host writer: fastp_amd.hostloop.apply_results, or fq_glue.cpp through its C entry points"""
    ref = mk_engine(params)
    n = fq1.count(b"\n") // 4
    if cpp_lib is None:
        want, _, _ = driver.run_engine(ref, params, fq1, fq2, pack=max(n, 1), stride=abi.qual_stride(max_len),
                                       want_failed=want_failed, want_unpaired=want_unpaired, umi=ed)
    else:
        want = _run_cpp_host(ref, params, fq1, fq2, abi.qual_stride(max_len), want_failed, want_unpaired, ed, cpp_lib)
    ref.close()
    return {k: bytes(getattr(want, k, None) or b"") for k in STREAMS}


class NamesCppHost(cpphost.CppHost):
    """cpphost.CppHost with the whole option word"""

    def __init__(self, lib, params, want_failed, want_unpaired, ed, word=None):
        self.lib = lib
        lib.fastp_gpu_host_output.restype = C.c_void_p
        lib.fastp_gpu_host_adapter_entries.restype = C.c_int64
        o = cpphost.HostOptions()
        o.want_failed, o.want_unpaired1, o.want_unpaired2 = int(want_failed), int(want_unpaired), int(want_unpaired)
        o.umi_loc = option_word(ed) if word is None else word
        if ed is not None:
            o.umi_len = ed.umi_len
            o.umi_prefix = ed.prefix or None
            o.umi_delimiter = ed.delimiter
        self.h = C.c_void_p()
        self.rc = lib.fastp_gpu_host_create(C.byref(params), C.byref(o), C.byref(self.h))
        self.params = params


def _run_cpp_host(engine, params, fq1, fq2, stride, want_failed, want_unpaired, ed, lib):
    b1 = hostloop.parse_fastq(fq1, stride)
    b2 = hostloop.parse_fastq(fq2, stride) if fq2 is not None else None
    host = NamesCppHost(lib, params, want_failed, want_unpaired, ed)
    assert host.rc == 0, host.rc
    if b2 is not None:
        r1, r2, pr, corr = engine.process(b1.seq, b1.qual, b1.lens, b2.seq, b2.qual, b2.lens)
    else:
        r1, r2, pr, corr = engine.process(b1.seq, b1.qual, b1.lens)
    host.apply(b1, b2, r1, r2, pr, corr, getattr(engine, "last_adapter_events", None))
    outs = host.outputs(b2 is not None)
    host.close()
    if not want_failed:
        outs.failed = None
    if not want_unpaired:
        outs.unpaired1 = outs.unpaired2 = None
    return outs


def capacities(n, t1, t2, ed, seven):
    """the bounds include/fastp_gpu.h documents for fastp_gpu_format_streams / fastp_gpu_format_all_streams"""
    D = G = 0
    if ed is not None and ed.loc:
        D = len(ed.delimiter) + (len(ed.prefix) + 1 if ed.prefix else 0)
        G = n * (D + 3) + t1 + t2 if ed.loc in LOCATIONS else n * (D + 2 * ed.umi_len + 1)
    both = t1 + t2 + 2 * (G + n) + 96 * n
    caps = [t1 + G + n, t2 + G + n, both, both, both, both]
    if seven:
        caps.append(t1 + G + n)
    return caps


def run_formatter(eng, mem, fq1, fq2, max_len, ed, seven, want_failed=True, want_unpaired=False, shrink=None, word=None,
                  shrink_to=100):
    """the text as one batch through fastp_gpu_format_streams (seven=False) or fastp_gpu_format_all_streams;
    returns (rc, {stream: bytes}, [needed lengths], [capacities]).  Buffers hold the documented bound (shrink: that stream's
    is declared as shrink_to bytes), are allocated 256 bytes longer than declared and are filled with 0xEE: nothing may be written past a stream's reported length."""
    c = f7.prepare(eng, mem, fq1, fq2, max_len)
    n, mates, res, paired = c["n"], c["mates"], c["res"], c["paired"]
    ios = []
    for m in range(2 if paired else 1):
        f = abi.FormatIn()
        f.text, f.line_off, f.line_len, f.res = (mem.ptr(mates[m]["text"]), mem.ptr(mates[m]["loff"]),
                                                 mem.ptr(mates[m]["llen"]), mem.ptr(res[m]))
        ios.append(f)
    o = abi.FormatOptions()
    o.want_failed, o.want_unpaired1, o.want_unpaired2 = int(want_failed), int(want_unpaired), int(want_unpaired)
    o.umi_loc = option_word(ed) if word is None else word
    if ed is not None:
        o.umi_len = ed.umi_len
        o.umi_prefix = ed.prefix or None
        o.umi_delimiter = ed.delimiter
    caps = capacities(n, mates[0]["nbytes"], mates[1]["nbytes"] if paired else 0, ed, seven)
    if shrink is not None:
        caps[shrink] = shrink_to
    outs = [mem.alloc(k + 256, 0xEE) for k in caps]   # (more than is declared: a write past a capacity lands in the fill)
    mem.sync()
    call = eng.format_all_streams if seven else eng.format_streams
    rc, lens = call(n, ios[0], ios[1] if paired else None, mem.ptr(c["pair"]) if paired else None, mem.ptr(c["corr"]),
                    mem.ptr(c["nc"]), o, [mem.ptr(x) for x in outs], caps, check=False)
    got = {}
    for i in range(len(caps)):
        whole = mem.download(outs[i])
        keep = min(lens[i], caps[i])
        got[STREAMS[i]] = whole[:keep]
        tail = whole[keep:]
        assert tail.count(b"\xEE") == len(tail), f"stream {STREAMS[i]}: bytes written past its length"
    return rc, got, lens, caps


def name_stats(want, fq1, fq2, ed):
    """what the EXPECTED streams hold, so that a pass is not vacuous: (tagged names, MGI-fixed names, names whose tag holds
    the MGI fix's space, names left without a tag) over every record of every stream"""
    orig = set(fq1.split(b"\n")[0::4]) | (set(fq2.split(b"\n")[0::4]) if fq2 else set())
    fixed = {hostloop.fix_mgi_name(x) for x in orig if hostloop.fix_mgi_name(x) != x} if ed is not None and ed.fix_mgi else set()
    tagged = mgi = inside = untagged = 0
    lead = (ed.delimiter + (ed.prefix + b"_" if ed.prefix else b"")) if ed is not None and ed.loc else None
    for k in STREAMS:
        for name in want[k].split(b"\n")[0::4][:-1]:
            if k == "merged" and b" merged_" in name:
                name = name[:name.rindex(b" merged_")]
            if k == "failed":
                name = name[:name.rindex(b" ")]
            if name in orig or name in fixed:
                untagged += 1
                if name in fixed:
                    mgi += 1
                continue
            tagged += 1
            if lead is not None and ed.fix_mgi:
                head = name.split(b" ")[0]
                rest = name[len(head):]
                if rest.count(b" /") >= 2:       # the tag ends in " /1" or " /2" and so does the name
                    inside += 1
                if name[-3:] in (b" /1", b" /2"):
                    mgi += 1
    return tagged, mgi, inside, untagged


# ---- the file loop (include/fastp_gpu_stream.h) with the whole option word ---------------------------------------------
def run_files(lib, params, in1, in2, outdir, want, chunk_bytes, ed, compress=(), device=0):
    """streamlib.run_files with the option word of an editor; returns (outputs: name -> bytes as written, counters, layout,
    AdapterMaps, StreamStats).  --overlapped_out's stream arrives through the emit callback (host assembly)."""
    paired = bool(params.paired)
    lib.fastp_gpu_stream_last_error.restype = C.c_char_p
    lib.fastp_gpu_stream_last_error.argtypes = [C.c_void_p]
    host = NamesCppHost(lib, params, "failed" in want, "unpaired1" in want, ed)
    assert host.rc == 0, host.rc
    cfg = streamlib.StreamConfig()
    cfg.in1 = in1.encode()
    cfg.in2 = in2.encode() if in2 else None
    cfg.chunk_bytes = chunk_bytes
    cfg.device = device
    cfg.format.want_failed = int("failed" in want)
    cfg.format.want_unpaired1 = int("unpaired1" in want)
    cfg.format.want_unpaired2 = int("unpaired2" in want)
    cfg.format.umi_loc = option_word(ed)
    if ed is not None:
        cfg.format.umi_len = ed.umi_len
        cfg.format.umi_prefix = ed.prefix or None
        cfg.format.umi_delimiter = ed.delimiter
    cfg.want_overlapped = int(bool(params.overlapped_out) and "overlapped" in want)
    fds, paths, collected = {}, {}, bytearray()
    for q, name in enumerate(streamlib.STREAM_NAMES):
        cfg.out_fd[q] = -1
        if name not in want or (not paired and q in (1, 3, 4, 5)):
            continue
        cfg.want[q] = 1
        cfg.compress[q] = int(name in compress)
        paths[q] = os.path.join(outdir, name + (".fq.gz" if name in compress else ".fq"))
        fds[q] = os.open(paths[q], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        cfg.out_fd[q] = fds[q]

    def on_emit(user, stream, data, n):
        if stream == streamlib.N_OUT and n:
            collected.extend(C.string_at(data, n))
        return 0
    cb = streamlib.EMIT_FN(on_emit)
    cfg.emit = cb
    cfg.host = host.h
    s = C.c_void_p()
    lib.fastp_gpu_stream_create.argtypes = [C.POINTER(abi.Params), C.POINTER(streamlib.StreamConfig), C.POINTER(C.c_void_p)]
    rc = lib.fastp_gpu_stream_create(C.byref(params), C.byref(cfg), C.byref(s))
    if rc != 0:
        host.close()
        for fd in fds.values():
            os.close(fd)
        raise streamlib.StreamError(rc, (lib.fastp_gpu_stream_last_error(None) or b"").decode())
    try:
        lib.fastp_gpu_stream_run.argtypes = [C.c_void_p]
        rc = lib.fastp_gpu_stream_run(s)
        if rc != 0:
            raise streamlib.StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        lay = abi.CounterLayout()
        lib.fastp_gpu_stream_layout.argtypes = [C.c_void_p, C.POINTER(abi.CounterLayout)]
        assert lib.fastp_gpu_stream_layout(s, C.byref(lay)) == 0
        ctr = np.zeros(lay.total, dtype=np.int64)
        lib.fastp_gpu_stream_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        rc = lib.fastp_gpu_stream_counters(s, ctr.ctypes.data, lay.total)
        if rc != 0:
            raise streamlib.StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        st = streamlib.StreamStats()
        lib.fastp_gpu_stream_get_stats.argtypes = [C.c_void_p, C.POINTER(streamlib.StreamStats)]
        lib.fastp_gpu_stream_get_stats(s, C.byref(st))
        amaps = host.adapter_maps()
    finally:
        lib.fastp_gpu_stream_destroy.argtypes = [C.c_void_p]
        lib.fastp_gpu_stream_destroy(s)
        host.close()
        for fd in fds.values():
            os.close(fd)
    outs = {name: open(paths[q], "rb").read() for q, name in enumerate(streamlib.STREAM_NAMES) if cfg.want[q]}
    if cfg.want_overlapped:
        outs["overlapped"] = bytes(collected)
    return outs, ctr, lay, amaps, st


# ---- fixtures recorded from the reference (tests/golden/read_names/make_fixtures.py) ----------------------------------
# T4's parameter sets: name -> (case of tests/cases.py whose flags and parameters are the base, the reference's extra flags,
# fields set on the parameters, editor arguments (loc, fix_mgi, prefix, delimiter))
FILE_SETS = {
    "pe_index1": ("pe_default", ["-U", "--umi_loc", "index1"], {}, ("index1", False, b"", b":")),
    "pe_index2": ("pe_cut_right", ["-U", "--umi_loc", "index2"], {}, ("index2", False, b"", b":")),
    "pe_per_index_prefix": ("pe_default", ["-U", "--umi_loc", "per_index", "--umi_prefix", "U", "--umi_delim", "#"], {},
                            ("per_index", False, b"U", b"#")),
    "pe_mgi": ("pe_default", ["--fix_mgi_id"], {}, (None, True, b"", b":")),
    "pe_per_index_mgi_merge": ("pe_merge", ["-U", "--umi_loc", "per_index", "--fix_mgi_id"], {}, ("per_index", True, b"", b":")),
    "se_index1": ("se_default_noadapter", ["-U", "--umi_loc", "index1"], {}, ("index1", False, b"", b":")),
    "se_per_index_mgi": ("se_adapter_cut", ["-U", "--umi_loc", "per_index", "--fix_mgi_id"], {}, ("per_index", True, b"", b":")),
}
N_FILE_RECORDS = 600


def file_set_inputs(name):
    """(paired, reference flags without / with the name options, fq1, fq2) of a T4 set"""
    case, extra_flags, _, _ = FILE_SETS[name]
    paired, flags, pf, skw = cases.CASES[case]
    d = synth.synth_pairs(N_FILE_RECORDS, L=150, seed=4321, paired=paired, **skw)
    fq1, fq2 = zoo_fastq(d, paired)
    return paired, list(flags), list(flags) + extra_flags, fq1, fq2


def file_set_params(name, max_len=152):
    case, _, fields, _ = FILE_SETS[name]
    p = cases.CASES[case][2](max_len)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def file_set_editor(name):
    loc, mgi, prefix, delim = FILE_SETS[name][3]
    return editor(loc, mgi, prefix, delim)


def load_file_set(name):
    """(fq1, fq2, meta) of tests/golden/read_names/<name>.npz; meta: outputs (md5, size), json, json_plain"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    meta = json.loads(z["meta"].tobytes().decode())
    return z["fq1"].tobytes(), (z["fq2"].tobytes() if "fq2" in z.files else None), meta


def load_table():
    """the reference's written names for the zoo: list of runs {loc, mgi, prefix, delimiter, paired, names1, names2}"""
    with open(os.path.join(GOLDEN_DIR, "names_table.json")) as f:
        t = json.load(f)
    assert [[a.decode("latin-1"), b.decode("latin-1")] for a, b in ZOO] == t["zoo"], "the table was recorded for another zoo"
    return t["runs"]
