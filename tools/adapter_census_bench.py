"""A stream run (include/fastp_gpu_stream.h) with FilterResult's adapter maps replayed on the host (the default) against the
adapter census on the device (fastp_gpu_stream_set_adapter_census): wall_s, replay_s, d2h_s, engine_s of the stream's own
statistics, `runs` runs each in turn on the same two plain files, after one warm-up run of each.  Input: synthetic 2x150 bp
pairs with the given mean insert size (below the read length most pairs are trimmed; tests/synth.py), 100 000 generated
pairs repeated to the wanted number, out1 + out2 written to files.

  adapter_census_bench.py [pairs] [insert_mean] [runs]     (defaults: 2000000 90 3)
  adapter_census_bench.py [pairs] [insert_mean] --once     one run with the census on, nothing else (for a kernel trace)"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + '/tests')
from fastp_amd import abi, engine   # noqa: E402
import census_util                  # noqa: E402
import synth                        # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
pairs = int(args[0]) if len(args) > 0 else 2000000
insert_mean = float(args[1]) if len(args) > 1 else 90.0
runs = int(args[2]) if len(args) > 2 else 3
once = "--once" in sys.argv
lib = engine.load_library(os.environ.get("FASTP_GPU_LIB"))
unit = min(pairs, 100000)
reps = max(1, pairs // unit)
d = synth.synth_pairs(unit, L=150, seed=7, paired=True, insert_mean=insert_mean, insert_sd=insert_mean / 3)
p = abi.default_params(True, 150)
with tempfile.TemporaryDirectory() as tmp:
    paths = []
    for m in (1, 2):
        paths.append(os.path.join(tmp, f"in{m}.fq"))
        with open(paths[-1], "wb") as f:
            text = synth.to_fastq(d[f"seq{m}"], d[f"qual{m}"], d[f"len{m}"], m)
            for _ in range(reps):
                f.write(text)

    def run(census):
        outs, ctr, lay, amaps, st, info = census_util.stream_run(lib, p, paths[0], paths[1], tmp, census=census)
        return st, amaps, ctr, lay

    def show(what, st):
        print(f"{what}: {st.units} pairs in {st.chunks} chunks; wall_s {st.wall_s:.3f} replay_s {st.replay_s:.3f} d2h_s {st.d2h_s:.3f} "
              f"engine_s {st.engine_s:.3f} (format_s {st.format_s:.3f} write_s {st.write_s:.3f} wait_read_s {st.wait_read_s:.3f})", flush=True)

    if once:
        st, amaps, _, _ = run(True)
        show("device census", st)
        sys.exit(0)
    st, host_maps, ctr, lay = run(False)
    trimmed = int(ctr[lay.adapter_reads])
    print(f"input: {st.units} pairs 2x150 bp, insert {insert_mean:.0f} +- {insert_mean / 3:.0f}; adapter-trimmed reads {trimmed} of {2 * st.units} "
          f"({100.0 * trimmed / (2 * st.units):.1f} %); map 1 / map 2 hold {len(host_maps.a1)} / {len(host_maps.a2)} keys", flush=True)
    st, dev_maps, _, _ = run(True)
    assert dev_maps.a1 == host_maps.a1 and dev_maps.a2 == host_maps.a2, "the census and the host replay disagree"
    for k in range(runs):
        show(f"host replay   run {k + 1}", run(False)[0])
        show(f"device census run {k + 1}", run(True)[0])
