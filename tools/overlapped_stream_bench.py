"""A stream run (include/fastp_gpu_stream.h) of an --overlapped_out job with the seventh stream assembled on the host
(the default) against the device path (fastp_gpu_stream_set_overlapped_output): wall_s, d2h_s, format_s, deflate_s of the
stream's own statistics, the second of two runs each.  Input: 20 000 synthetic 2x150 bp pairs whose read 1 reaches past
the overlap (no adapter trimming), repeated `reps` times, as two plain files in a temporary directory.

  overlapped_stream_bench.py [reps] [--gz]     --gz: the seventh stream compressed on the device (device path only)"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + '/tests')
from fastp_amd import abi, engine
import streamlib, streamlib7, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 50
lib = engine.load_library()
d = synth.synth_pairs(20000, L=150, seed=1, paired=True, insert_mean=150.0, insert_sd=60.0)
p = abi.default_params(True, 150)
p.overlapped_out, p.adapter_enabled = 1, 0
want = ("out1", "out2", "failed", "overlapped")
with tempfile.TemporaryDirectory() as tmp:
    paths = []
    for m in (1, 2):
        paths.append(os.path.join(tmp, f"in{m}.fq"))
        with open(paths[-1], "wb") as f:
            text = synth.to_fastq(d[f"seq{m}"], d[f"qual{m}"], d[f"len{m}"], m)
            for _ in range(reps):
                f.write(text)

    def show(what, st, nbytes):
        print(f"{what}: {st.units} pairs in {st.chunks} chunks, {nbytes/1e6:.1f} MB overlapped; wall_s {st.wall_s:.3f} d2h_s {st.d2h_s:.3f} "
              f"format_s {st.format_s:.3f} deflate_s {st.deflate_s:.3f} (engine_s {st.engine_s:.3f} write_s {st.write_s:.3f})", flush=True)

    texts = {}
    for run in range(2):
        outs, _, _, _, st = streamlib.run_files(lib, p, paths[0], paths[1], tmp, want=want, emit=False)
        texts["host"] = outs["overlapped"]
    show("host path (emit)      ", st, st.bytes_overlapped)
    for how in ("emit", "fd") + (("gz",) if "--gz" in sys.argv else ()):
        for run in range(2):
            outs, _, _, _, st, info = streamlib7.run_files(lib, p, paths[0], paths[1], tmp, want=want, overlapped=how)
        assert info["on_device"] == 1
        if how != "gz":
            assert outs["overlapped"] == texts["host"], "the device path wrote other bytes"
        show(f"device path ({how:4s})    ", st, st.bytes_overlapped)
    # without the adapter replay's host object the records and line tables stay on the device
    for run in range(2):
        outs, _, _, _, st, info = streamlib7.run_files(lib, p, paths[0], paths[1], tmp, want=want, overlapped="fd", with_host=False)
    assert outs["overlapped"] == texts["host"]
    show("device path (fd, no replay)", st, st.bytes_overlapped)
