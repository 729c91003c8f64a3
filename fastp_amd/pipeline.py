"""FASTQ files in -> trimmed / filtered FASTQ files out, every per-read step on the device.

The host only moves bytes: it reads raw text chunks (the reference's FastqReader fills 8 MiB blocks,
fastqreader.cpp:31,88-149), ships them to HBM, and writes the text that comes back (WriterThread,
writerthread.cpp:118-168).  Line splitting + packing (`fastp_gpu_parse_fastq`), the worker loop
(`fastp_gpu_submit_device`) and record formatting (`fastp_gpu_format_fastq`) run on the GPU; what the
reference's processSingleEnd / processPairEnd would have written to out1 / out2 comes out byte for
byte.  Input files may be plain FASTQ or BGZF (.gz written by bgzip: the reference's BgzfMtReader path,
src/bgzf.h) - those are shipped compressed and inflated on the device (`fastp_gpu_inflate_bgzf`).
Every output stream of the worker loop is assembled on the device (`fastp_gpu_format_streams`; with `--overlapped_out`
`fastp_gpu_format_all_streams`, which writes that option's stream as well): out1 / out2,
--failed_out, --unpaired1/2, the merged stream, UMI-renamed records; an output path ending in ".gz" is compressed
on the device too (`fastp_gpu_deflate_bgzf`: BGZF-framed gzip members, what the reference's WriterThread does per
pack with libdeflate).  Reader and writer run on their own threads so file I/O overlaps the device work of the
neighbouring chunks.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import time

import numpy as np

from . import abi, engine


class PipelineError(RuntimeError):
    pass


class _Mate:
    """per-mate buffers of one in-flight chunk"""

    def __init__(self, torch, dev, text, max_records, max_len):
        ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
        self.cap = text.numel()                   # [text carried from the previous chunk | this chunk's text]
        self.text = text
        self.seq = torch.empty(max_records * ss, dtype=torch.uint8, device=dev)
        self.qual = torch.empty(max_records * qs, dtype=torch.uint8, device=dev)
        self.lens = torch.empty(max_records, dtype=torch.int16, device=dev)
        self.loff = torch.empty(4 * max_records, dtype=torch.int32, device=dev)
        self.llen = torch.empty(4 * max_records, dtype=torch.int32, device=dev)
        self.res = torch.zeros(max_records * 12, dtype=torch.uint8, device=dev)


class FastqPipeline:
    def __init__(self, params: abi.Params, device: int = 0, chunk_bytes: int = 256 << 20, max_records: int | None = None,
                 corr_capacity: int = 1 << 22):
        import torch
        self.torch = torch
        self.params = params
        self.paired = bool(params.paired)
        self.dev = torch.device("cuda", device)
        self.eng = engine.GpuEngine(params, device=device)
        self.chunk = int(chunk_bytes)
        self.max_records = int(max_records or max(1024, (2 * self.chunk) // 48))
        nm = 2 if self.paired else 1
        # one allocation for both mates' text (and, for BGZF input, one for their compressed chunks): a single
        # inflate launch then covers the blocks of both files
        self.text_cap = (2 * self.chunk + 64 + 255) // 256 * 256
        self.text_all = torch.zeros(nm * self.text_cap, dtype=torch.uint8, device=self.dev)
        self.comp_cap = (self.chunk + 64 + 255) // 256 * 256
        self.comp_all = None
        self.idx_all = None
        self.mates = [_Mate(torch, self.dev, self.text_all[m * self.text_cap:(m + 1) * self.text_cap], self.max_records,
                            params.max_len) for m in range(nm)]
        self.pair = torch.zeros(self.max_records * 8, dtype=torch.uint8, device=self.dev)
        self.corr_cap = corr_capacity if params.correction else 0
        self.corr = torch.zeros(max(1, self.corr_cap) * 8, dtype=torch.uint8, device=self.dev)
        self.nc = torch.zeros(4, dtype=torch.int32, device=self.dev)
        nf = int(params.n_adapter_fasta)
        self.ev_cap = self.max_records * 2 * min(nf, 8) if nf else 0
        self.ev = torch.zeros(max(1, self.ev_cap) * 12, dtype=torch.uint8, device=self.dev)
        self.nev = torch.zeros(4, dtype=torch.int32, device=self.dev)
        # two pinned staging sets per direction: the reader fills one while the device works on the other
        self.stage_in = [[torch.empty(self.chunk + 64, dtype=torch.uint8).pin_memory() for _ in range(nm)] for _ in range(2)]
        self.stage_out = None      # [slot][stream]: pinned, sized in run() for the streams that are asked for
        # (seven streams: --overlapped_out's is the last, written when params.overlapped_out is set)
        self.outs = [None] * abi.N_ALL_OUTPUTS   # device text per stream
        self.gzbuf = [None] * abi.N_ALL_OUTPUTS  # device gzip members per compressed stream
        self.gz_level = None                     # run(compression_level=...)
        self.max_blocks = (2 * self.chunk) // 8192 + 64     # BGZF members per chunk (bgzip: ~64 KiB of text each)
        self.check_crc = True
        self.stats = dict(units=0, chunks=0, bytes_in=0, bytes_out=0, t_parse=0.0, t_engine=0.0, t_format=0.0, t_h2d=0.0,
                          t_d2h=0.0, t_wait_read=0.0, t_wait_write=0.0)

    def close(self):
        self.eng.close()

    # -- reader thread: (leftover of the previous chunk | fresh bytes) into a pinned staging buffer ------------
    IO_THREADS = int(os.environ.get("FASTP_PIPELINE_IO_THREADS", "8"))   # positional reads / writes in flight per direction
    IO_PIECE = 32 << 20

    def _reader(self, files, q_free, q_full, tails):
        """fills a staging set: [file bytes the last trip left over | fresh bytes], all mates concurrently;
        tails[m] = bytes per trip for file m"""
        import os
        from concurrent.futures import ThreadPoolExecutor
        fds = [f.fileno() for f in files]
        sizes = [os.fstat(fd).st_size for fd in fds]
        pos = [0] * len(files)

        def piece(fd, mv, off):
            got = 0
            while got < len(mv):
                r = os.preadv(fd, [mv[got:]], off + got)
                if r <= 0:
                    raise PipelineError("short read")
                got += r

        try:
            with ThreadPoolExecutor(self.IO_THREADS) as pool:
                while True:
                    item = q_free.get()
                    if item is None:
                        return
                    slot, carry, budget = item
                    fills, futs = [], []
                    for m in range(len(files)):
                        buf = self.stage_in[slot][m].numpy()
                        k = len(carry[m])
                        if k:
                            buf[:k] = np.frombuffer(carry[m], dtype=np.uint8)
                        want = max(0, min(budget[m] - k, sizes[m] - pos[m]))
                        mv = memoryview(buf)[k:k + want]
                        for a in range(0, want, self.IO_PIECE):
                            e = min(want, a + self.IO_PIECE)
                            futs.append(pool.submit(piece, fds[m], mv[a:e], pos[m] + a))
                        pos[m] += want
                        fills.append((k + want, pos[m] >= sizes[m]))
                    for fu in futs:
                        fu.result()
                    q_full.put((slot, fills))
        except Exception as e:  # surface in the main thread
            q_full.put(e)

    def _writer(self, files, q_out, q_done):
        import os
        from concurrent.futures import ThreadPoolExecutor
        fds = [f.fileno() if f is not None else -1 for f in files]
        pos = [0] * len(files)

        def piece(fd, mv, off):
            done = 0
            while done < len(mv):
                done += os.pwritev(fd, [mv[done:]], off + done)

        try:
            with ThreadPoolExecutor(self.IO_THREADS) as pool:
                while True:
                    item = q_out.get()
                    if item is None:
                        return
                    slot, lens = item[0], item[1]
                    futs = []
                    closing = []
                    for file_no, close, spans in (item[2] if len(item) > 2 else ()):   # split outputs: the trip's pieces by file
                        sw = self._split_w
                        if sw["open"] != file_no:
                            self._split_open(file_no)
                        for q, (off, ln) in enumerate(spans):
                            if sw["fd"][q] < 0 or not ln:
                                continue
                            mv = memoryview(self.stage_out[slot][q].numpy())[off:off + ln]
                            for a in range(0, ln, self.IO_PIECE):
                                futs.append(pool.submit(piece, sw["fd"][q], mv[a:min(ln, a + self.IO_PIECE)], sw["pos"][q] + a))
                            sw["pos"][q] += ln
                        if close:
                            closing += [fd for fd in sw["fd"] if fd >= 0]
                            sw["fd"], sw["open"] = [-1, -1], 0
                    for m in range(len(files)):
                        if files[m] is None or not lens[m]:
                            continue
                        mv = memoryview(self.stage_out[slot][m].numpy())[:lens[m]]
                        for a in range(0, lens[m], self.IO_PIECE):
                            e = min(lens[m], a + self.IO_PIECE)
                            futs.append(pool.submit(piece, fds[m], mv[a:e], pos[m] + a))
                        pos[m] += lens[m]
                    for fu in futs:
                        fu.result()
                    for fd in closing:
                        os.close(fd)
                    q_done.put(slot)
        except Exception as e:
            q_done.put(e)

    # ---- --split / --split_by_lines: the one worker's file state (src/threadconfig.cpp:106-157), as fq_stream.cpp keeps it ----
    @staticmethod
    def split_name(out: str, file_no: int, digits: int) -> str:
        """dirname(out) / (number, zero-padded to `digits`) + "." + basename(out)"""
        import os
        d, b = os.path.split(out)
        return os.path.join(d, str(file_no).rjust(digits, "0") + "." + b)

    def _split_open(self, file_no):
        import os
        sp, sw = self._split, self._split_w
        for q, out in enumerate(sp["out"]):
            sw["fd"][q] = os.open(self.split_name(out, file_no, sp["digits"]), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            sw["pos"][q] = 0
        sw["open"] = file_no

    def _split_pack_done(self):
        """ThreadConfig::markProcessed after a pack; True = the next file was opened"""
        sp = self._split
        sp["current"] += sp["pack_passed"] if sp["by_lines"] else sp["pack_units"]
        sp["pack_units"] = sp["pack_passed"] = 0
        if sp["current"] >= sp["size"] and (sp["by_lines"] or sp["working"] + 1 < sp["number"]):
            sp["working"] += 1
            sp["files"] += 1
            sp["current"] = 0
            return True
        return False

    def _split_pieces(self, n, passed):
        """the trip's packs through the state machine: [(file, closes, first table entry, entry behind the last)]"""
        sp = self._split
        pieces, begin, i, u, end_all = [], 0, 0, sp["units"], sp["units"] + n
        while u < end_all:
            end = min(end_all, (u // abi.PACK_SIZE + 1) * abi.PACK_SIZE)
            sp["pack_units"] += end - u
            sp["pack_passed"] += int(passed[i])
            u, i = end, i + 1
            if end % abi.PACK_SIZE:
                break                      # the pack goes on in the next trip (or is the input's last)
            file_no = sp["working"] + 1
            if self._split_pack_done():
                pieces.append((file_no, True, begin, i))
                begin = i
        slices = (end_all - 1) // abi.PACK_SIZE - sp["units"] // abi.PACK_SIZE + 1
        if begin < slices:
            pieces.append((sp["working"] + 1, False, begin, slices))
        sp["units"] = end_all
        return pieces

    def _split_finish(self):
        """behind the last trip: the input's last pack (short or empty; it may open one more file), by-number mode's files that
        were never reached (writeEmptyFilesForSplitting); every file still open or never created is finished"""
        import os
        sp, sw = self._split, self._split_w
        todo = [sp["working"] + 1]
        if self._split_pack_done():
            todo.append(sp["working"] + 1)
        while not sp["by_lines"] and sp["working"] + 1 < sp["number"]:
            sp["working"] += 1
            sp["files"] += 1
            todo.append(sp["working"] + 1)
        for file_no in todo:
            if sw["open"] != file_no:
                self._split_open(file_no)
            for q, fd in enumerate(sw["fd"]):
                if fd < 0:
                    continue
                if self.gz_out[q]:
                    os.pwrite(fd, self.EOF_MEMBER, sw["pos"][q])
                os.close(fd)
            sw["fd"], sw["open"] = [-1, -1], 0

    @staticmethod
    def is_bgzf(path: str) -> bool:
        """isBgzf (src/bgzf.h:17-27): gzip magic, FEXTRA, BC subfield of length 2 first"""
        with open(path, "rb") as f:
            h = f.read(18)
        return (len(h) == 18 and h[0] == 0x1f and h[1] == 0x8b and h[2] == 8 and (h[3] & 4) and h[12] == 0x42 and h[13] == 0x43
                and (h[14] | (h[15] << 8)) == 2)

    def _inflate_all(self, slot, fills, tcarry, gz):
        """BGZF bytes in the staging buffers -> text on the device behind each mate's carried text, ONE launch for
        the blocks of all compressed mates.  Returns per mate (text bytes added, compressed bytes consumed)."""
        torch = self.torch
        nm = len(self.mates)
        if self.comp_all is None:
            self.comp_all = torch.zeros(nm * self.comp_cap, dtype=torch.uint8, device=self.dev)
            self.idx_all = torch.zeros(nm * self.max_blocks * 24 + 64, dtype=torch.uint8, device=self.dev)
        res = [(0, 0)] * nm
        parts = [[] for _ in range(5)]
        for m in range(nm):
            if not gz[m]:
                continue
            nb, eof_file = fills[m]
            host = self.stage_in[slot][m].numpy()[:nb]
            room = self.mates[m].cap - 64 - tcarry[m]
            info, poff, plen, isz, crc, ooff = self.eng.bgzf_index(host, self.max_blocks, room)
            nblk, used = int(info.n_blocks), int(info.consumed)
            if nblk == 0:
                if eof_file and nb > 0:
                    raise PipelineError(f"truncated BGZF member at the end of mate {m + 1}'s file")
                continue
            c0 = m * self.comp_cap
            self.comp_all[c0:c0 + used].copy_(self.stage_in[slot][m][:used], non_blocking=True)
            self.comp_all[c0 + used:c0 + used + 32].zero_()
            parts[0].append(poff + np.uint32(c0))
            parts[1].append(plen)
            parts[2].append(isz)
            parts[3].append(crc)
            parts[4].append(ooff + np.uint64(m * self.text_cap + tcarry[m]))
            res[m] = (int(info.out_bytes), used)
        n = sum(len(a) for a in parts[0])
        if n == 0:
            return res
        packed = np.concatenate([np.concatenate(p).view(np.uint8) for p in parts])   # 4+4+4+4+8 bytes per block
        self.idx_all[:packed.size].copy_(torch.from_numpy(packed), non_blocking=False)
        base = self.idx_all.data_ptr()
        torch.cuda.synchronize(self.dev)
        self.eng.inflate_bgzf(self.comp_all.data_ptr(), n, base, base + 4 * n, base + 8 * n, base + 12 * n, base + 16 * n,
                              self.text_all.data_ptr(), self.text_all.numel(), self.check_crc)
        return res

    EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # bgzip's empty last member

    def _setup_outputs(self, paths, umi=None, fix_mgi_id=False, interleaved=False, split=False):
        """device + pinned buffers for the streams that are written; paths[q] per abi stream index"""
        torch = self.torch
        nm = len(self.mates)
        # what a record can grow by over its input text: the UMI name tag (addUmiToName: delimiter + prefix + '_' + the
        # UMI of one or both mates joined by '_'), the failed / merged tags on the name and the strand line.  A tag taken
        # from the names' indexes is as long as those: over a chunk such tags add up to less than the text of both mates
        # (fastp_gpu_format_streams' bound); the MGI fix adds a byte per record
        grow = names = 0
        if umi:
            grow = len(umi[3] if len(umi) > 3 and umi[3] else b":") + (len(umi[2]) + 1 if len(umi) > 2 and umi[2] else 0)
            if umi[0] in ("index1", "index2", "per_index"):
                grow += 3
                names = nm * self.text_cap
            else:
                grow += 2 * int(umi[1]) + 1
        if fix_mgi_id:
            grow += 1
        both = nm * self.text_cap + 2 * names + self.max_records * (96 + 2 * grow)   # every record of both mates + tags
        one = self.text_cap + names + self.max_records * (64 + grow)
        # --overlapped_out's stream: parts of read 1's records + the name edit (fastp_gpu_format_all_streams' bound)
        # (out1 as --stdout's interleaved stream holds both mates' records: fastp_gpu_format_interleaved's bound)
        caps = [both if interleaved else one, one, both, both, both, both, self.text_cap + names + self.max_records * grow]
        self.out_cap = [0] * abi.N_ALL_OUTPUTS
        self.gz_out = [bool(p) and p.endswith(".gz") for p in paths]
        for q in range(abi.N_ALL_OUTPUTS):
            if not paths[q]:
                continue
            self.out_cap[q] = caps[q]
            if self.outs[q] is None or self.outs[q].numel() < caps[q]:
                self.outs[q] = torch.empty(caps[q], dtype=torch.uint8, device=self.dev)
            if self.gz_out[q]:
                gcap = caps[q] + 31 * (caps[q] // 65280 + 1) + 64
                if split:   # a segment per pack of the trip, each with a last member and maybe an end-of-file member
                    gcap += (31 + 28) * (self.max_records // abi.PACK_SIZE + 3)
                if self.gzbuf[q] is None or self.gzbuf[q].numel() < gcap:
                    self.gzbuf[q] = torch.empty(gcap, dtype=torch.uint8, device=self.dev)
        need = [(self.gzbuf[q].numel() if self.gz_out[q] else caps[q]) if paths[q] else 0 for q in range(abi.N_ALL_OUTPUTS)]
        if self.stage_out is None:
            self.stage_out = [[None] * abi.N_ALL_OUTPUTS for _ in range(2)]
        for sl in range(2):
            for q in range(abi.N_ALL_OUTPUTS):
                have = self.stage_out[sl][q]
                if need[q] and (have is None or have.numel() < need[q]):
                    self.stage_out[sl][q] = torch.empty(need[q], dtype=torch.uint8).pin_memory()

    def run(self, in1: str, in2: str | None, out1: str, out2: str | None, failed_out: str | None = None,
            merged_out: str | None = None, unpaired1: str | None = None, unpaired2: str | None = None,
            umi: tuple | None = None, compression_level: int | None = None, overlapped_out: str | None = None,
            fix_mgi_id: bool = False, adapter_counts: bool = False, interleaved_out: bool = False, split: tuple | None = None,
            split_digits: int = 4) -> dict:
        """umi = (location "read1" | "read2" | "per_read", length[, prefix bytes[, delimiter bytes]]): the name edit that goes
        with params.umi_len1/2 (UmiProcessor::addUmiToName); or (location "index1" | "index2" | "per_index", 0[, prefix[,
        delimiter]]): the UMI is the index part of the name, nothing is trimmed.  fix_mgi_id: --fix_mgi_id, a space in front
        of a name's final /1 or /2, before the UMI edit.  compression_level: the reference's -z (1..9, 0 = the default)
        for every ".gz" output; None is the default encoder through fastp_gpu_deflate_bgzf.  overlapped_out: the file of
        --overlapped_out's stream, needed when params.overlapped_out is set (a ".gz" path is compressed like the others).
        adapter_counts: FilterResult's adapter-string maps (the report's adapter_cutting.read1_adapter_counts /
        read2_adapter_counts) are counted on the device, per chunk, on the tensors the chunk already holds
        (fastp_gpu_adapter_census); adapter_counts() returns them.
        interleaved_out: --stdout of a paired run without merge (src/peprocessor.cpp:577-585): out1 receives both records of a
        passing pair, read 1's first; out2 must be None.
        split: ("lines", L) for --split_by_lines L, or ("files", N, reads_per_file) for --split N (reads_per_file: the input's
        read count / N, the reference's estimate); split_digits: --split_prefix_digits.  out1 / out2 are then the name
        templates: file k is dirname / (k padded to split_digits) + "." + basename, ".gz" names are compressed and every file
        ends in bgzip's end-of-file member; as in the reference no other stream is written and merge / interleaved_out are
        refused (src/threadconfig.cpp:106-157, the same rules as fastp_gpu_stream_set_split); stats["split_files"] = the files
        opened per stream"""
        self.census = bool(adapter_counts)
        torch = self.torch
        if compression_level is not None and not 0 <= int(compression_level) <= 9:
            raise PipelineError("compression_level is 0 (the default) to 9")
        self.gz_level = None if compression_level is None else int(compression_level)
        if interleaved_out:
            if not self.paired or self.params.merge:
                raise PipelineError("interleaved_out (--stdout) is the stream of a paired run without merge")
            if out2 is not None or not out1:
                raise PipelineError("interleaved_out (--stdout): out1 receives the stream, out2 must be None")
            if split is not None:
                raise PipelineError("--split cannot be combined with interleaved_out (--stdout)")
        if self.paired != (in2 is not None) or (self.paired != (out2 is not None) and not interleaved_out):
            raise PipelineError("paired engine needs in2/out2, single-end engine must not get them")
        self._split, self._pieces = None, []
        if split is not None:
            if self.params.merge:
                raise PipelineError("--split cannot be combined with --merge")
            for name, v in (("failed_out", failed_out), ("merged_out", merged_out), ("unpaired1", unpaired1), ("unpaired2", unpaired2),
                            ("overlapped_out", overlapped_out)):
                if v:
                    raise PipelineError(f"--split writes out1 / out2 only: the reference drops {name} in this mode")
            if not isinstance(split, tuple) or not split or split[0] not in ("lines", "files") or len(split) != (2 if split[0] == "lines" else 3):
                raise PipelineError('split is ("lines", L) or ("files", N, reads_per_file)')
            by_lines = split[0] == "lines"
            if by_lines and (int(split[1]) % 4 or int(split[1]) < 4):
                raise PipelineError("--split_by_lines: a multiple of 4 lines")
            size = int(split[1]) // 4 if by_lines else int(split[2])
            if size < 1:
                raise PipelineError("--split / --split_by_lines: reads_per_file below 1")
            if not by_lines and not 2 <= int(split[1]) <= 999:
                raise PipelineError("--split: number outside 2..999")
            if not 0 <= int(split_digits) <= 10:
                raise PipelineError("--split_prefix_digits outside 0..10")
            if not out1:
                raise PipelineError("--split: out1 is missing")
            self._split = dict(by_lines=by_lines, size=size, number=0 if by_lines else int(split[1]), digits=int(split_digits),
                               out=[out1, out2] if self.paired else [out1], units=0, working=0, current=0, pack_units=0,
                               pack_passed=0, files=1, max_packs=self.max_records // abi.PACK_SIZE + 2)
            self._split_w = dict(fd=[-1, -1], pos=[0, 0], open=0)
            mp = self._split["max_packs"]
            self._split["cut"] = torch.zeros(2 * (mp + 1), dtype=torch.int64, device=self.dev)
            self._split["passed"] = torch.zeros(mp, dtype=torch.int32, device=self.dev)
        if self.paired and not self.params.merge:
            self.eng.format_interleaved(bool(interleaved_out))
        if self.params.merge and not merged_out:
            raise PipelineError("merge mode needs merged_out")
        if bool(self.params.overlapped_out) != bool(overlapped_out):
            raise PipelineError("params.overlapped_out and the overlapped_out file go together")
        if (self.params.umi_len1 or self.params.umi_len2) and umi is None:
            raise PipelineError("params trim a UMI off the reads: pass umi=(location, length) for the name edit")
        out_paths = [out1, out2, failed_out, merged_out if self.params.merge else None, unpaired1 if self.paired else None,
                     unpaired2 if self.paired else None, overlapped_out]
        self._setup_outputs(out_paths, umi, fix_mgi_id, bool(interleaved_out), split is not None)
        self.fmt_opts = abi.FormatOptions()
        self.fmt_opts.want_failed = int(bool(failed_out))
        self.fmt_opts.want_unpaired1 = int(bool(out_paths[4]))
        self.fmt_opts.want_unpaired2 = int(bool(out_paths[5]))
        if umi is not None:
            if umi[0] not in abi.UMI_LOC:
                raise PipelineError(f"unknown UMI location {umi[0]!r}")
            self.fmt_opts.umi_loc = abi.UMI_LOC[umi[0]]
            self.fmt_opts.umi_len = int(umi[1])
            self.fmt_opts.umi_prefix = umi[2] if len(umi) > 2 and umi[2] else None
            self.fmt_opts.umi_delimiter = umi[3] if len(umi) > 3 else None
        if fix_mgi_id:
            self.fmt_opts.umi_loc |= abi.NAME_FIX_MGI
        nm = len(self.mates)
        paths = (in1, in2) if self.paired else (in1,)
        gz = [self.is_bgzf(p) for p in paths]
        for p, g in zip(paths, gz):
            if not g:
                with open(p, "rb") as f:
                    if f.read(2) == b"\x1f\x8b":
                        raise PipelineError(f"{p}: gzip but not BGZF - a single deflate stream has no independent blocks; "
                                            "decompress on the host (as the reference does) or recompress with bgzip")
        fin = [open(p, "rb", buffering=0) for p in paths]
        # (split outputs: out1 / out2 are name templates, the writer opens the files)
        fout = [open(p, "wb", buffering=0) if p and not (self._split and q < 2) else None for q, p in enumerate(out_paths)]
        finished = False
        q_free, q_full, q_out, q_done = queue.Queue(), queue.Queue(), queue.Queue(), queue.Queue()
        # a compressed chunk expands ~4-5x: read a quarter of the text budget per trip
        want = [self.chunk // 4 if g else self.chunk for g in gz]
        rd = threading.Thread(target=self._reader, args=(fin, q_free, q_full, want), daemon=True)
        wr = threading.Thread(target=self._writer, args=(fout, q_out, q_done), daemon=True)
        rd.start()
        wr.start()
        st = self.stats
        st.setdefault("t_inflate", 0.0)
        t_start = time.perf_counter()
        tcarry = [0] * nm          # text bytes already at the front of mates[m].text (device-side carry)
        try:
            q_free.put((0, [b""] * nm, list(want)))
            out_free = [0, 1]
            done = False
            drain = False              # every file is at EOF but the device still holds complete records
            slot = 0
            while not done:
                if drain:
                    fills = [(0, True)] * nm   # nothing new from the files: parse what was carried over
                else:
                    t0 = time.perf_counter()
                    item = q_full.get()
                    if isinstance(item, Exception):
                        raise item
                    slot, fills = item
                    st["t_wait_read"] += time.perf_counter() - t0
                st["bytes_in"] += sum(f[0] for f in fills)
                total, fcarry, eof = [0] * nm, [b""] * nm, [False] * nm
                if any(gz):
                    t0 = time.perf_counter()
                    inflated = self._inflate_all(slot, fills, tcarry, gz)
                    st["t_inflate"] += time.perf_counter() - t0
                for m in range(nm):
                    nb, eof_file = fills[m]
                    M = self.mates[m]
                    if gz[m]:
                        added, used = inflated[m]
                        if nb > used:
                            fcarry[m] = bytes(memoryview(self.stage_in[slot][m].numpy())[used:nb])
                        if added == 0 and not eof_file and len(fcarry[m]) >= want[m]:
                            raise PipelineError("the text buffer cannot take another BGZF block: raise chunk_bytes")
                        total[m] = tcarry[m] + added
                        eof[m] = eof_file and not fcarry[m]
                    else:
                        t0 = time.perf_counter()
                        if tcarry[m] + nb > M.cap - 64:
                            raise PipelineError("a record does not fit the chunk size")
                        M.text[tcarry[m]:tcarry[m] + nb].copy_(self.stage_in[slot][m][:nb], non_blocking=True)
                        torch.cuda.synchronize(self.dev)
                        st["t_h2d"] += time.perf_counter() - t0
                        total[m] = tcarry[m] + nb
                        eof[m] = eof_file
                    M.text[total[m]:total[m] + 32].zero_()
                all_eof = all(eof)
                # ---- parse (both mates to the same record count) ----
                t0 = time.perf_counter()
                infos = [self._parse(m, total[m], eof[m], self.max_records) for m in range(nm)]
                n = min(i.n_records for i in infos)
                for m in range(nm):
                    if infos[m].n_records != n:
                        infos[m] = self._parse(m, total[m], eof[m], n)
                st["t_parse"] += time.perf_counter() - t0
                left = [total[m] - int(infos[m].consumed) for m in range(nm)]
                # the reader refills the other staging set while the device works on this chunk; a plain-text mate
                # whose tail stays on the device gets that much less this trip
                if not all_eof:
                    q_free.put((1 - slot, fcarry, [want[m] if gz[m] else max(0, want[m] - left[m]) for m in range(nm)]))
                if all_eof:
                    # a trip takes at most max_records records: when the cap was hit, complete records may remain in
                    # the carried text - keep parsing without refilling until a trip comes back short.  What is left
                    # then is a trailing partial record / the longer mate's surplus: the reference stops too
                    drain = n > 0 and n >= self.max_records and any(left)
                    done = not drain
                elif n == 0 and any(left[m] >= self.chunk for m in range(nm)):
                    raise PipelineError("a record does not fit the chunk size")
                if n > 0:
                    lens = self._process_and_format(n, st)
                    # ---- D2H + hand to the writer ----
                    t0 = time.perf_counter()
                    while not out_free:
                        d = q_done.get()
                        if isinstance(d, Exception):
                            raise d
                        out_free.append(d)
                    st["t_wait_write"] += time.perf_counter() - t0
                    oslot = out_free.pop(0)
                    t0 = time.perf_counter()
                    for q in range(abi.N_ALL_OUTPUTS):
                        if (fout[q] is not None or (self._split and q < 2)) and lens[q]:
                            src = self.gzbuf[q] if self.gz_out[q] else self.outs[q]
                            self.stage_out[oslot][q][:lens[q]].copy_(src[:lens[q]], non_blocking=True)
                    torch.cuda.synchronize(self.dev)
                    st["t_d2h"] += time.perf_counter() - t0
                    q_out.put((oslot, lens, self._pieces) if self._split else (oslot, lens))
                    st["units"] += n
                    st["chunks"] += 1
                    st["bytes_out"] += sum(lens)
                # ---- the unconsumed text tail moves to the front (after formatting: the records point into the text) ----
                for m in range(nm):
                    a = int(infos[m].consumed)
                    if left[m] and a:
                        tail = self.mates[m].text[a:total[m]].clone()
                        self.mates[m].text[:left[m]].copy_(tail)
                    tcarry[m] = left[m]
            finished = True
        finally:
            q_free.put(None)
            q_out.put(None)
            wr.join()
            rd.join(timeout=5)
            if self._split:   # (the writer thread has joined: its file state is ours)
                if finished:
                    self._split_finish()
                for fd in self._split_w["fd"]:
                    if fd >= 0:
                        os.close(fd)
                st["split_files"] = self._split["files"]
            for q, f in enumerate(fout):
                if f is not None and self.gz_out[q]:   # the writer thread has joined: append after its last positional write
                    os.pwrite(f.fileno(), self.EOF_MEMBER, os.fstat(f.fileno()).st_size)
            for f in fin + fout:
                if f is not None:
                    f.close()
        while not q_done.empty():
            d = q_done.get()
            if isinstance(d, Exception):
                raise d
        st["wall"] = time.perf_counter() - t_start
        return dict(st)

    def _process_and_format(self, n, st):
        """worker loop + record formatting of the parsed chunk; returns the output byte counts per stream"""
        nm = len(self.mates)
        t0 = time.perf_counter()
        b = abi.Batch()
        b.n, b.flags = n, abi.BATCH_STAT_ISIZE
        M = self.mates
        b.seq1, b.qual1, b.len1 = M[0].seq.data_ptr(), M[0].qual.data_ptr(), M[0].lens.data_ptr()
        if self.paired:
            b.seq2, b.qual2, b.len2 = M[1].seq.data_ptr(), M[1].qual.data_ptr(), M[1].lens.data_ptr()
        xu = np.unique(np.concatenate([getattr(M[m], "exotic", np.zeros(0, dtype=np.int32)) for m in range(nm)])).astype(np.int32)
        xu = np.ascontiguousarray(xu[xu < n])
        if len(xu):
            b.n_exotic, b.exotic_dense, b.exotic_unit = len(xu), 1, xu.ctypes.data
            for m in range(nm):
                b.exotic_text[m], b.exotic_off[m] = M[m].text.data_ptr(), M[m].loff.data_ptr()
        r = abi.Results()
        r.r1 = M[0].res.data_ptr()
        if self.paired:
            r.r2, r.pair = M[1].res.data_ptr(), self.pair.data_ptr()
        if self.corr_cap:
            r.corrections, r.corrections_capacity = self.corr.data_ptr(), self.corr_cap
        r.n_corrections = self.nc.data_ptr()
        if self.ev_cap:
            r.adapter_events, r.adapter_events_capacity, r.n_adapter_events = self.ev.data_ptr(), self.ev_cap, self.nev.data_ptr()
        self.eng.submit_device(b, r)
        self.eng.synchronize()
        if self.corr_cap and int(self.nc[0].item()) > self.corr_cap:   # before anything reads the list
            raise PipelineError("correction list overflow: raise corr_capacity")
        st["t_engine"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        fi = []
        for m in range(nm):
            f = abi.FormatIn()
            f.text, f.line_off, f.line_len, f.res = M[m].text.data_ptr(), M[m].loff.data_ptr(), M[m].llen.data_ptr(), M[m].res.data_ptr()
            fi.append(f)
        sp = self._split
        if sp:   # the pack table of this trip: where out1 / out2 may change files
            plan = abi.PackCuts()
            plan.first_unit, plan.pack_size, plan.max_packs = sp["units"], abi.PACK_SIZE, sp["max_packs"]
            plan.cut, plan.passed = sp["cut"].data_ptr(), sp["passed"].data_ptr()
            self.eng.format_pack_cuts(plan)
        # the six streams of the worker loop, or all seven for an --overlapped_out run
        ns = abi.N_ALL_OUTPUTS if self.params.overlapped_out else abi.N_OUTPUTS
        fmt = self.eng.format_all_streams if self.params.overlapped_out else self.eng.format_streams
        rc, lens = fmt(n, fi[0], fi[1] if self.paired else None, self.pair.data_ptr() if self.paired else None,
                       self.corr.data_ptr() if self.corr_cap else None, self.nc.data_ptr() if self.corr_cap else None, self.fmt_opts,
                       [t.data_ptr() if t is not None and self.out_cap[q] else None for q, t in enumerate(self.outs[:ns])],
                       self.out_cap[:ns])
        lens += [0] * (abi.N_ALL_OUTPUTS - ns)
        if self.corr_cap and int(self.nc[0].item()) > self.corr_cap:
            raise PipelineError("correction list overflow: raise corr_capacity")
        st["t_format"] += time.perf_counter() - t0
        st["bytes_text"] = st.get("bytes_text", 0) + sum(lens)
        if self.census:
            t0 = time.perf_counter()
            self.eng.adapter_census(n, fi[0], fi[1] if self.paired else None, self.corr.data_ptr() if self.corr_cap else None,
                                    self.nc.data_ptr() if self.corr_cap else None, self.corr_cap,
                                    self.ev.data_ptr() if self.ev_cap else None, self.nev.data_ptr() if self.ev_cap else None, self.ev_cap)
            st["t_census"] = st.get("t_census", 0.0) + time.perf_counter() - t0
        t0 = time.perf_counter()
        if sp:
            cut = sp["cut"].cpu().numpy().reshape(2, sp["max_packs"] + 1)
            ranges = self._split_pieces(n, sp["passed"].cpu().numpy())
            spans = [[(0, 0)] * len(sp["out"]) for _ in ranges]
            for q in range(len(sp["out"])):
                seg_off = [int(cut[q][r[2]]) for r in ranges] + [int(cut[q][ranges[-1][3]])]
                if self.gz_out[q]:   # one call for the trip: a segment per piece, the end-of-file member behind a file that ends
                    rc, seg_off = self.eng.deflate_bgzf_segments(self.outs[q].data_ptr(), seg_off, [r[1] for r in ranges], self.gz_level or 0,
                                                                 self.gzbuf[q].data_ptr(), self.gzbuf[q].numel())
                    lens[q] = seg_off[-1]
                for k in range(len(ranges)):
                    spans[k][q] = (seg_off[k], seg_off[k + 1] - seg_off[k])
            self._pieces = [(r[0], r[1], spans[k]) for k, r in enumerate(ranges)]
        for q in range(abi.N_ALL_OUTPUTS):
            if self.out_cap[q] and self.gz_out[q] and not (sp and q < 2):
                rc, lens[q] = self.eng.deflate_bgzf(self.outs[q].data_ptr(), lens[q], self.gzbuf[q].data_ptr(), self.gzbuf[q].numel(),
                                                          level=self.gz_level)
        st["t_deflate"] = st.get("t_deflate", 0.0) + time.perf_counter() - t0
        return lens

    def _parse(self, m, nbytes, is_last, max_records):
        M = self.mates[m]
        info = self.eng.parse_fastq(M.text.data_ptr(), nbytes, is_last, max_records, M.seq.data_ptr(), M.qual.data_ptr(),
                                    M.lens.data_ptr(), M.loff.data_ptr(), M.llen.data_ptr())
        if info.first_bad >= 0:
            raise PipelineError(f"malformed FASTQ record {info.first_bad} of a chunk (mate {m + 1}): the device parser does not repair input")
        # records with letters outside ACGTN: the engine's text kernel takes those units from the chunk's own text
        M.exotic = self.eng.parse_exotic() if info.n_exotic else np.zeros(0, dtype=np.int32)
        return info

    def counters(self):
        return self.eng.counters()

    def adapter_counts(self):
        """FilterResult::mAdapter1 / mAdapter2 of the runs made with adapter_counts=True: an object with the two dicts
        {adapter bytes: count} as .a1 / .a2 (hostloop.AdapterMaps), in the reference's map order"""
        from . import hostloop
        m = hostloop.AdapterMaps()
        m.a1, m.a2 = self.eng.adapter_counts(False), self.eng.adapter_counts(True)
        return m
