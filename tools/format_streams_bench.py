"""Time of the device stream formatter on tools/format_bench.py's input (20 000 synthetic 2x150 bp pairs, repeated):
parse -> submit_device -> fastp_gpu_format_streams, every buffer resident in HBM; one warm-up call, then five timed ones,
their median and spread.

  format_streams_bench.py [reps]                  the six-stream call (runs against any build of the library: FASTP_GPU_LIB)
  format_streams_bench.py [reps] --overlapped     --overlapped_out input without adapter trimming (read 1 reaches past the
                                                  overlap): the six-stream call (the caller declares that it writes the
                                                  seventh stream itself) next to fastp_gpu_format_all_streams
  format_streams_bench.py [reps] --names index1|per_index|mgi
                                                  the six-stream call on the same records with umi_loc 0, per_read (8 bases)
                                                  and the named option (mgi: --fix_mgi_id alone, on names that end in a dual
                                                  index and /1, /2 instead of " 1:N:0:ATCG")
  ... --names X --variant loc0|per_read|named     only one of the three, for a kernel trace of its own"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + '/tests')
import numpy as np, torch
from fastp_amd import abi, engine
import synth

names = sys.argv[sys.argv.index("--names") + 1] if "--names" in sys.argv else None
assert names in (None, "index1", "per_index", "mgi")
variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
assert variant in (None, "loc0", "per_read", "named")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (names, variant)]
overlapped = "--overlapped" in sys.argv
reps = int(args[0]) if args else 50
dev = torch.device('cuda', 0)
n0 = 20000
p = abi.default_params(True, 150)
if overlapped:
    d = synth.synth_pairs(n0, L=150, seed=1, paired=True, insert_mean=150.0, insert_sd=60.0)
    p.overlapped_out, p.adapter_enabled = 1, 0
else:
    d = synth.synth_pairs(n0, L=150, seed=1, paired=True)
    p.correction = 1
g = engine.GpuEngine(p)
n = n0 * reps
ss, qs = abi.seq_stride(150), abi.qual_stride(150)
mates = []
for m in (1, 2):
    text = synth.to_fastq(d[f"seq{m}"], d[f"qual{m}"], d[f"len{m}"], m)
    if names == "mgi":
        text = text.replace(b" %d:N:0:ATCG\n" % m, b":ATCGAATT+GGTACCAA/%d\n" % m)
    text = text * reps
    pad = (-len(text)) % 16 + 16
    t = torch.frombuffer(bytearray(text + b"\0" * pad), dtype=torch.uint8).to(dev)
    seq = torch.empty((n, ss), dtype=torch.uint8, device=dev); qual = torch.empty((n, qs), dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.int16, device=dev)
    loff = torch.empty(4 * n, dtype=torch.int32, device=dev); llen = torch.empty(4 * n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    info = g.parse_fastq(t.data_ptr(), len(text), True, n, seq.data_ptr(), qual.data_ptr(), lens.data_ptr(), loff.data_ptr(), llen.data_ptr())
    assert info.n_records == n
    mates.append(dict(t=t, seq=seq, qual=qual, lens=lens, loff=loff, llen=llen, nbytes=len(text)))
res = [torch.zeros(n * 12, dtype=torch.uint8, device=dev) for _ in range(2)]
pr = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
cap = 1 << 22
corr = torch.zeros(cap * 8, dtype=torch.uint8, device=dev); nc = torch.zeros(1, dtype=torch.int32, device=dev)
b = abi.Batch(); b.n, b.flags = n, abi.BATCH_STAT_ISIZE
b.seq1, b.qual1, b.len1 = (mates[0][k].data_ptr() for k in ("seq", "qual", "lens"))
b.seq2, b.qual2, b.len2 = (mates[1][k].data_ptr() for k in ("seq", "qual", "lens"))
r = abi.Results(); r.r1, r.r2, r.pair = res[0].data_ptr(), res[1].data_ptr(), pr.data_ptr()
r.corrections, r.corrections_capacity, r.n_corrections = corr.data_ptr(), cap, nc.data_ptr()
torch.cuda.synchronize()
g.submit_device(b, r); g.synchronize()
fin = []
for m in range(2):
    f = abi.FormatIn(); f.text, f.line_off, f.line_len, f.res = mates[m]["t"].data_ptr(), mates[m]["loff"].data_ptr(), mates[m]["llen"].data_ptr(), res[m].data_ptr()
    fin.append(f)
o = abi.FormatOptions(); o.want_failed = 1
total = mates[0]["nbytes"] + mates[1]["nbytes"]
grow = 64 if names else 0   # per record: the longest tag here is ":" + 8 + "_" + 8 bases, or two 8-base indexes with the MGI space
caps = [mates[0]["nbytes"] + n * grow + 64, mates[1]["nbytes"] + n * grow + 64, total + n * (64 + 2 * grow), 0, 0, 0, mates[0]["nbytes"]]
outs = [torch.empty(max(16, c), dtype=torch.uint8, device=dev) if c else None for c in caps]
ptrs = [t.data_ptr() if t is not None else None for t in outs]
torch.cuda.synchronize()


def timed(what, call):
    ms = []
    for it in range(6):   # the first call is the warm-up
        t0 = time.perf_counter()
        rc, lens = call()
        dt = (time.perf_counter() - t0) * 1e3
        if it:
            ms.append(dt)
    med = statistics.median(ms)
    print(f"{what}: {n} pairs, {sum(lens)/1e6:.1f} MB out ({', '.join(str(x) for x in lens)}); " +
          " ".join(f"{x:.2f}" for x in ms) + f" ms; median {med:.2f} ms, spread {min(ms):.2f}..{max(ms):.2f} ms, "
          f"{sum(lens)/med/1e6:.2f} GB/s written", flush=True)


if overlapped:
    g.lib.fastp_gpu_host_writes_overlapped.argtypes = [C.c_void_p, C.c_int]
    g.lib.fastp_gpu_host_writes_overlapped(g.h, 1)
if names:
    for key, what, word, ul in (("loc0", "umi_loc 0", 0, 0), ("per_read", "per_read, 8 bases", abi.UMI_PER_READ, 8),
                                ("named", names, {"index1": abi.UMI_INDEX1, "per_index": abi.UMI_PER_INDEX, "mgi": abi.NAME_FIX_MGI}[names], 0)):
        if variant not in (None, key):
            continue
        o.umi_loc, o.umi_len = word, ul
        timed(f"fastp_gpu_format_streams, {what:18s}", lambda: g.format_streams(n, fin[0], fin[1], pr.data_ptr(), corr.data_ptr(), nc.data_ptr(), o, ptrs[:6], caps[:6]))
    sys.exit(0)
timed("fastp_gpu_format_streams    ", lambda: g.format_streams(n, fin[0], fin[1], pr.data_ptr(), corr.data_ptr(), nc.data_ptr(), o, ptrs[:6], caps[:6]))
if overlapped:
    timed("fastp_gpu_format_all_streams", lambda: g.format_all_streams(n, fin[0], fin[1], pr.data_ptr(), corr.data_ptr(), nc.data_ptr(), o, ptrs, caps))
