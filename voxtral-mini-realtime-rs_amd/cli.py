"""`voxtral-transcribe`-compatible driver (reference: src/bin/transcribe.rs:27-318): same flags, one line of text per
input on stdout, logs on stderr.  WAV ingest / resampling / chunking / token decode stay on the CPU (caller side in the
reference too); pad -> log-mel -> encoder -> decoder run on the GPU through the C ABI.

    python -m ... cli --gguf model.gguf --tokenizer tekken.json --audio a.wav [--audio b.wav] [--delay 6] [--max-mel-frames 1200]
"""
from __future__ import annotations

import argparse
import sys
import time
import wave

import numpy as np


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def load_wav(path):
    """audio/io.rs:90-131: PCM int (8/16/24/32 bit, hound's i32 samples) mixed to mono as (sum of the channels as f32 / channels) / 2^(bits-1);
    IEEE float: mean of the channels."""
    with wave.open(path, "rb") as w:
        ch, sw, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if sw == 2:
        v = np.frombuffer(raw, dtype="<i2").astype(np.int64)
    elif sw == 4:
        v = np.frombuffer(raw, dtype="<i4").astype(np.int64)
    elif sw == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16); v = np.where(v & 0x800000, v - (1 << 24), v)
    elif sw == 1:
        v = np.frombuffer(raw, dtype=np.uint8).astype(np.int64) - 128            # hound: 8-bit WAV is unsigned, read as signed
    else:
        raise ValueError(f"unsupported WAV sample width {sw}")
    s = v.reshape(-1, ch).sum(axis=1) if ch > 1 else v                            # i32 sum of the frame's channels (io.rs:110-113)
    x = (s.astype(np.float32) / np.float32(ch)) / np.float32(1 << (8 * sw - 1))
    return x.astype(np.float32), sr


def resample_to_16k(x, sr, ctx=None, pkg=None):
    """audio/resample.rs:10-52.  vox_resample on the GPU: the algorithm of rubato's synchronous FFT resampler, which is what the reference calls
    (tests/test_resample.py pins it against the CPU oracle's independent restatement; the crate itself is outside the reference's tree, so parity with ITS
    output is unpinned and recorded as such in DESIGN.md).  There is no host fallback: without the HIP library this CLI cannot resample."""
    if ctx is None or pkg is None:
        raise RuntimeError("resample_to_16k needs a GPU context (the product path has no CPU fallback)")
    return pkg.resample_to_16k(ctx, x, sr)


def unit_words(pkg, path, chunk, ids, scores, tokenizer, alternatives=None):
    """--words: the words of one unit of work (a file, or chunk `chunk` of a chunked file; None: the file is one unit) as dicts: pkg.words' text, first_id, last_id
    (indices into the UNIT's ids), logprob, min_margin, with alternatives also entropy and weakest; + file and, for a chunk, chunk.  No due_s: that is when a live
    session hands an id out."""
    res = []
    for w in pkg.words(ids, scores, tokenizer, alternatives=alternatives):
        w = {k: v for k, v in w.items() if k != "due_s"}; w["file"] = path
        if chunk is not None:
            w["chunk"] = int(chunk)
        res.append(w)
    return res


def write_word_lines(out, lines):
    """one JSON line per word dict"""
    import json
    for w in lines:
        out.write(json.dumps(w, ensure_ascii=False) + "\n")
    out.flush()


def transcribe_one(pkg, path, model, tokenizer, mel, pad_cfg, chunk_cfg, t_embed, words_out=None, alts_k=0):
    """bin/transcribe.rs:187-276.  words_out (--words): every chunk's logits rows come back with its ids and vox_records_rows' kernel gives every id its record
    (alts_k: --alternatives); the ids, hence the line, are the same."""
    x, sr = load_wav(path)
    if sr != 16000:
        log(f"  resampling {sr} Hz -> 16 kHz"); x = resample_to_16k(x, sr, mel.ctx, pkg)
    x = pkg.peak_normalize(x, 0.95)                                              # :207
    chunks = pkg.chunk_audio(x, chunk_cfg) if pkg.needs_chunking(x.size, chunk_cfg) else [None]
    texts = []; words = []
    for i, ch in enumerate(chunks):
        samples = x if ch is None else ch.samples
        if len(chunks) > 1:
            log(f"  chunk {i + 1}/{len(chunks)}: {ch.start_sample / 16000:.2f}-{ch.end_sample / 16000:.2f} s")
        m = mel.compute_log(pkg.pad_audio(samples, pad_cfg))                     # :279-306
        if m.shape[0] == 0:
            raise RuntimeError("Audio too short to produce mel frames")
        if words_out is None:
            ids = model.transcribe_streaming(np.ascontiguousarray(m.T)[None], t_embed)
        else:
            ids, lg = model.transcribe_streaming(np.ascontiguousarray(m.T)[None], t_embed, return_logits=True)
            if len(ids):
                sc, al = pkg.records_rows(mel.ctx, lg, alts_k)
                words.extend(unit_words(pkg, path, i if len(chunks) > 1 else None, ids, sc, tokenizer, al))
        text = tokenizer.decode([t for t in ids if t >= 1000]).strip()           # :309-318
        if text:
            texts.append(text)
    if words_out is not None:      # (a file that failed half way writes nothing)
        write_word_lines(words_out, words)
    return " ".join(texts)


def write_words(out, pkg, path, ids, scores, tokenizer, rate, alternatives=None, delay=None, levels=None):
    """--live-words: one JSON line per word of a file that has ended (pkg.words: text, first_id, last_id, due_s, logprob, min_margin) + the file's path; with
    --live-alternatives also the word's entropy and the alternatives of its weakest id; delay (--live-delays): the delay of the member that ran the file; with
    --live-levels also peak_db and rms_db -- null where the level has no finite dB figure: digital silence (a level of 0 is -inf dB) or an id without a record, so that
    every line stays strict JSON."""
    import json
    import math
    for w in pkg.words(ids, scores, tokenizer, sample_rate=rate, alternatives=alternatives, levels=levels):
        if levels is not None:
            w = dict(w, peak_db=w["peak_db"] if math.isfinite(w["peak_db"]) else None, rms_db=w["rms_db"] if math.isfinite(w["rms_db"]) else None)
        w = dict(w, file=path) if delay is None else dict(w, file=path, delay=int(delay))
        out.write(json.dumps(w, ensure_ascii=False) + "\n")
    out.flush()


class Endpoint:
    """--live-endpoint-ms MS [--live-endpoint-db DB]: one session's end-of-speech trigger on its quiet_ticks.  due(ids_out, quiet) is True once per quiet run -- the
    maximal run of quiet records that ends at the last id -- when the run has reached MS; a non-quiet (or missing) record starts the next run, which re-arms it."""

    def __init__(self, ms, db):
        self.ms, self.db, self.fired = ms, db, None

    def due(self, ids_out, quiet):
        run = ids_out - quiet      # the id the run began at
        if quiet == 0 or quiet * 160 < self.ms or self.fired == run:
            return False
        self.fired = run
        return True


def transcribe_live(pkg, path, model, tokenizer, mel, t_embed, chunk_ms, native_rate=False, words_out=None, peek=False, alts_k=0, endless=False, suspend_every=0, burst=0, levels=False,
                    endpoint_ms=0, endpoint_db=-50.0):
    """--live: the file through a live session (vox_stream) in pieces of `chunk_ms` milliseconds, the text so far on stderr whenever ids arrive.  The gain is the
    file's peak scale 0.95 / max|x| (bin/transcribe.rs:207; a file is known in advance -- a microphone caller passes its own), the whole file is one utterance (no
    --max-mel-frames chunks: the session's state is bounded by its ring), so the line equals the un-chunked path's.
    native_rate (--live-native-rate), for a file that is not at 16 kHz: the session is created for the file's rate and pushed the file's own samples -- what a capture
    device would deliver; it resamples as the samples arrive.  The gain stays the peak scale of the RESAMPLED file (computed here only because the file is known in
    advance and the line is to be compared), so the line equals the one without the flag.
    words_out (--live-words): the session runs with scores on and the file's words go there when it ends; the ids, hence the line, are the same.
    alts_k (--live-alternatives): the session also keeps every id's alts_k best alternatives and the step's entropy, for the words file.
    peek (--live-peek): after every push a "  ~[" line on stderr with the text so far plus the tentative tail -- what the line would be if the file ended here
    (vox_stream_peek: finish's ticks, taken back); the session, hence everything else, is as without the flag.
    endless (--live-endless): the session is an endless one (vox_stream_create_endless: no 43-minute limit, the decoder cache a ring); the line is the same.
    suspend_every (--live-suspend-every N): after every N pushes the session is snapshotted to host memory (vox_stream_snapshot), the stream is freed, and a fresh one
    is restored from the blob (vox_stream_restore) -- what a server does with a caller on hold; the line is the same.
    burst (--live-burst B): the session is a burst stream (vox_stream_create_burst): a chunk longer than a tick runs its ticks in bursts of up to B; the line is the
    same up to near-ties, and depends on --live-chunk-ms up to near-ties.
    levels (--live-levels): the session runs with levels on (vox_stream_set_levels) and every --live-words line carries peak_db and rms_db.
    endpoint_ms / endpoint_db (--live-endpoint-ms, --live-endpoint-db; levels are on): after a push whose quiet time (quiet_ticks x 160 ms below endpoint_db) has reached
    endpoint_ms, ONE peek per quiet run prints the tentative "  ~[" line as --live-peek does; the session goes on, the next non-quiet record re-arms the trigger."""
    x, sr = load_wav(path)
    rate = 16000
    if sr != 16000:
        log(f"  resampling {sr} Hz -> 16 kHz"); x16 = resample_to_16k(x, sr, mel.ctx, pkg)
        if native_rate:
            rate = sr; log(f"  live session at {sr} Hz: the resampled file gives the gain alone")
        else:
            x = x16
    else:
        x16 = x
    x = np.ascontiguousarray(x, dtype=np.float32)
    peak = np.float32(np.abs(x16).max()) if x16.size else np.float32(0)
    gain = float(np.float32(0.95) / peak) if peak >= 1e-10 else 1.0              # audio/io.rs:59-68
    step = max(1, int(round(rate * chunk_ms / 1000.0)))
    def create():
        st = model.create_stream(t_embed, gain=gain, sample_rate=rate, endless=endless, burst=burst or None)
        if words_out is not None:
            st.set_scores(True)
            if alts_k:
                st.set_alternatives(alts_k)
        if levels:
            st.set_levels(True)
        return st
    stream = create()
    endpoint = Endpoint(endpoint_ms, endpoint_db) if endpoint_ms else None
    try:
        ids = []
        text = lambda tail=(): tokenizer.decode([t for t in ids + [int(v) for v in tail] if t >= 1000]).strip()   # :309-318
        for a in range(0, x.size, step):
            new = stream.push(x[a:a + step])
            if new.size:
                ids.extend(int(t) for t in new); log(f"  [{min(a + step, x.size) / rate:8.2f} s] {text()}")
            if peek:
                log(f"  ~[{min(a + step, x.size) / rate:8.2f} s] {text(stream.peek())}")
            elif endpoint is not None and endpoint.due(len(ids), stream.quiet_ticks(endpoint.db)):
                log(f"  ~[{min(a + step, x.size) / rate:8.2f} s] {text(stream.peek())}")
            if suspend_every and (a // step + 1) % suspend_every == 0:
                blob = stream.snapshot(); stream.close()
                stream = create(); stream.restore(blob)
                log(f"  *[{min(a + step, x.size) / rate:8.2f} s] suspended to {blob.size} bytes and resumed in a fresh stream")
        ids.extend(int(t) for t in stream.finish())
        if words_out is not None:
            write_words(words_out, pkg, path, ids, stream.scores(), tokenizer, rate, stream.alternatives() if alts_k else None, levels=stream.levels() if levels else None)
        return text()
    finally:
        stream.close()


def parse_live_delays(text, n_members):
    """--live-delays: "6,10,..." -> one integer delay (>= 0) per member; a single value serves every member.  ValueError when a value is no such integer or the count
    is neither 1 nor n_members."""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        delays = [int(p) for p in parts]
    except ValueError:
        raise ValueError(f"--live-delays takes integers separated by commas, got {text!r}") from None
    if any(d < 0 for d in delays):
        raise ValueError(f"--live-delays takes delays >= 0, got {text!r}")
    if len(delays) not in (1, n_members):
        raise ValueError(f"--live-delays names {len(delays)} delays for {n_members} members: one per member, or one for all")
    return delays * n_members if len(delays) == 1 else delays


def transcribe_live_group(pkg, paths, model, tokenizer, mel, t_embed, chunk_ms, n_members, words_out=None, peek=False, alts_k=0, page_rows=None, pool_pages=None, endless=False,
                          suspend_every=0, kv_dtype=None, delays=None, levels=False, endpoint_ms=0, endpoint_db=-50.0):
    """(levels / endpoint_ms / endpoint_db: as transcribe_live's, per member -- the members whose trigger is due after a call share one group peek.)
    (delays, --live-delays: one delay per member -- the group is made by vox_stream_group_create_t_embeds, member k's files run at delays[k], and every --live-words
    line gains "delay"; None: every member at t_embed.)
    (kv_dtype, --live-kv f32 | bf16: the paged group's K/V pool dtype, vox_stream_group_create_kv; the lines have the same form.)
    --live-group N: the files N at a time through one stream group (vox_stream_group) in pieces of `chunk_ms` milliseconds: every call feeds each busy member its
    next piece, a file that ends (its member fed with finish) frees the member for the next file in input order.  Gains and lines as transcribe_live's (16 kHz: other
    rates are resampled first).  -> {file index: text}; a file that cannot be read is left out (the one-by-one path reports it).  words_out (--live-words): every
    member runs with scores on (and, with alts_k from --live-alternatives, with that many alternatives), a file's words go there when the file ends.  peek (--live-peek): after every call one vox_stream_group_peek for the members still
    busy, a "  ~[" line each: the text so far plus the tentative tail.  page_rows / pool_pages (--live-page-rows, --live-pool-pages): either one given makes the group a
    paged one (vox_stream_group_create_paged); the lines are the same.  endless (--live-endless): the group is an endless paged one (vox_stream_group_create_endless: no
    member is refused at 43 minutes); the lines are the same.  suspend_every (--live-suspend-every N): after every N calls each busy member is snapshotted to host
    memory, reset, and restored from its blob (vox_stream_group_snapshot / _restore); the lines are the same."""
    step = max(1, int(round(16000 * chunk_ms / 1000.0)))
    group = model.create_stream_group(None if delays else t_embed, n_members, page_rows=page_rows, pool_pages=pool_pages, endless=endless, kv_dtype=kv_dtype, delays=delays)
    text = lambda ids: tokenizer.decode([t for t in ids if t >= 1000]).strip()
    texts = {}; busy = {}; nxt = 0; calls = 0      # busy: member -> [file index, samples, offset, ids]
    endpoints = {}      # member -> its file's Endpoint
    try:
        for k in range(n_members if levels else 0):
            group.set_levels(k, True)
        for k in range(n_members if words_out is not None else 0):
            group.set_scores(k, True)
            if alts_k:
                group.set_alternatives(k, alts_k)
        while nxt < len(paths) or busy:
            for k in range(n_members):
                while k not in busy and nxt < len(paths):
                    i = nxt; nxt += 1
                    try:
                        x, sr = load_wav(paths[i])
                        if sr != 16000:
                            x = resample_to_16k(x, sr, mel.ctx, pkg)
                    except Exception as e:
                        log(f"Error reading {paths[i]}: {e}"); continue
                    x = np.ascontiguousarray(x, dtype=np.float32)
                    peak = np.float32(np.abs(x).max()) if x.size else np.float32(0)
                    group.reset(k, float(np.float32(0.95) / peak) if peak >= 1e-10 else 1.0)      # audio/io.rs:59-68
                    busy[k] = [i, x, 0, []]
                    if endpoint_ms:
                        endpoints[k] = Endpoint(endpoint_ms, endpoint_db)
            if not busy:
                break
            feeds = {k: b[1][b[2]:b[2] + step] for k, b in busy.items()}
            last = [k for k, b in busy.items() if b[2] + step >= b[1].size]
            for k, new in group.advance(feeds, finish=last).items():
                b = busy[k]; b[2] += step
                if new.size:
                    b[3].extend(int(t) for t in new); log(f"  [{paths[b[0]]} {min(b[2], b[1].size) / 16000:8.2f} s] {text(b[3])}")
            for k in last:
                b = busy.pop(k); texts[b[0]] = text(b[3])
                if words_out is not None:
                    write_words(words_out, pkg, paths[b[0]], b[3], group.scores(k), tokenizer, 16000, group.alternatives(k) if alts_k else None, delay=delays[k] if delays else None,
                                levels=group.levels(k) if levels else None)
            ended = [] if peek or not endpoint_ms else [k for k in sorted(busy) if endpoints[k].due(len(busy[k][3]), group.quiet_ticks(k, endpoint_db))]
            for k, tail in (group.peek(sorted(busy)) if peek and busy else group.peek(ended) if ended else {}).items():
                b = busy[k]; log(f"  ~[{paths[b[0]]} {min(b[2], b[1].size) / 16000:8.2f} s] {text(b[3] + [int(v) for v in tail])}")
            calls += 1
            for k in (sorted(busy) if suspend_every and calls % suspend_every == 0 else []):
                blob = group.snapshot(k); group.reset(k, 1.0); group.restore(k, blob)
        return texts
    finally:
        group.close()


def file_costs(paths):
    """Decode cost of a file ~ its duration (the reference has no early stop): the file size is the proxy that needs no decode."""
    import os
    return [float(os.path.getsize(p)) if os.path.exists(p) else 0.0 for p in paths]


def unit_table(pkg, paths, chunk_cfg):
    """The units of work of a file list, from the WAV headers alone (so every rank derives the same table without decoding anything): every file is split exactly like
    bin/transcribe.rs:210-226 -- one unit if it fits `max_mel_frames`, its chunks otherwise -- at the length it will have at 16 kHz.
    -> [(file index, chunk index, start_sample, end_sample)], file-major.  Unreadable / empty files contribute nothing: their line (and their error) comes from the
    one-by-one path."""
    units = []
    for i, p in enumerate(paths):
        try:
            with wave.open(p, "rb") as w:
                n, sr = w.getnframes(), w.getframerate()
            n16 = pkg.resample_len(n, sr) if sr != 16000 else n
            if n16 <= 0:
                continue
            plan = pkg.chunk_plan(n16, chunk_cfg) if pkg.needs_chunking(n16, chunk_cfg) else [(0, n16)]
            units.extend((i, k, a, b) for k, (a, b) in enumerate(plan) if b > a)
        except Exception:
            pass
    return units


class UnitRunner:
    """Transcribes units (file, chunk, start, end) through vox_transcribe_batch_ex.  A file is loaded, resampled and peak-normalised ONCE, as a file
    (bin/transcribe.rs:197-207); its chunks are views into it handed over as already normalised (norm_group < 0), so a file's chunks may sit in different calls or
    on different ranks and still carry the file's scale.  Returns the text of every unit (None = failed: the file falls back to the one-by-one path).
    alts_k (--words: 0 = scores alone, 1..8 with --alternatives; None: off): the units go through vox_transcribe_batch_scored and self.words[(file, chunk)] holds
    every unit's word dicts (unit_words), for the caller to write once the file's line stands."""

    def __init__(self, pkg, ctx, model, tokenizer, paths, t_embed, alts_k=None, chunked=()):
        self.pkg, self.ctx, self.model, self.tok, self.paths, self.t_embed = pkg, ctx, model, tokenizer, paths, t_embed
        self.files = {}; self.alts_k = alts_k; self.chunked = set(chunked); self.words = {}

    def samples(self, i):
        if i not in self.files:
            try:
                x, sr = load_wav(self.paths[i])
                if sr != 16000:
                    x = resample_to_16k(x, sr, self.ctx, self.pkg)
                self.files[i] = self.pkg.peak_normalize(x, 0.95)
            except Exception as e:
                log(f"  (batched path) cannot read {self.paths[i]}: {e}"); self.files[i] = None
        return self.files[i]

    def __call__(self, units):
        views, keep = [], []
        for u, (i, k, a, b) in enumerate(units):
            x = self.samples(i)
            if x is not None and b <= x.size:      # (a header that lied about the length: leave the file to the one-by-one path)
                views.append(x[a:b]); keep.append(u)
        out = [None] * len(units)
        if not views:
            return out
        try:
            t1 = time.time()
            if self.alts_k is None:
                ids = self.model.transcribe_batch(views, self.t_embed, norm_group=[-1] * len(views))
            else:
                ids, scs, als = self.model.transcribe_batch_scored(views, self.t_embed, alternatives=self.alts_k, norm_group=[-1] * len(views))
            log(f"batch of {len(views)}: {time.time() - t1:.3f}s")
            for j, (u, r) in enumerate(zip(keep, ids)):
                out[u] = self.tok.decode([t for t in r if t >= 1000]).strip()           # :309-318, per chunk
                if self.alts_k is not None:
                    i, k = units[u][0], units[u][1]
                    self.words[(i, k)] = unit_words(self.pkg, self.paths[i], k if i in self.chunked else None, r, scs[j], self.tok, None if als is None else als[j])
        except Exception as e:
            log(f"batched path failed ({e}); falling back to one by one")
        for i in {units[u][0] for u in keep}:      # a file whose units are all done is dropped from memory
            self.files.pop(i, None)
        return out


def join_units(n_files, units, unit_texts):
    """bin/transcribe.rs:261-275: a file's line = its non-empty chunk texts joined by one space.  -> {file index: line} for the files whose units ALL came back."""
    per = {}
    for (i, k, _, _), t in zip(units, unit_texts):
        per.setdefault(i, []).append((k, t))
    lines = {}
    for i, lst in per.items():
        if all(t is not None for _, t in lst):
            lines[i] = " ".join(t for _, t in sorted(lst) if t)
    return lines


def _gloo_gather(fn):
    """Run `fn(group)` -- which ends in ONE gather of python objects -- over a GLOO group whatever the default group is: with `--gguf --gpus N` the default group is
    RCCL (the start-up weight broadcast), whose object collectives stage through GPU buffers and fall under the NCCL watchdog's 10-minute collective timeout -- a rank
    that is still transcribing a long share must not be killed by the ranks that wait for it.  Every rank calls this, so every rank takes part in new_group."""
    import datetime
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", timeout=datetime.timedelta(hours=12))
    sub = None
    try:
        group = None
        if not own and dist.get_backend() != "gloo":
            sub = dist.new_group(backend="gloo", timeout=datetime.timedelta(hours=12)); group = sub
        return fn(group)
    finally:
        if sub is not None:
            dist.destroy_process_group(sub)
        if own:
            dist.barrier(); dist.destroy_process_group()


def sharded_lines(pkg, paths, one, rank, world, group=None):
    """N > 1 ranks: every rank transcribes its longest-first share of `paths` with `one(index) -> text`; rank 0 returns every line in input order
    (None elsewhere).  The only collective is the final gather of the text lines (over gloo: _gloo_gather)."""
    if group is not None:
        return pkg.shard.run_sharded(list(range(len(paths))), file_costs(paths), one, rank, world, group=group)
    return _gloo_gather(lambda g: pkg.shard.run_sharded(list(range(len(paths))), file_costs(paths), one, rank, world, group=g))


def sharded_units(pkg, units, runner, batch, rank, world, group=None):
    """N > 1 ranks, chunks as units of work: the units are LPT-partitioned by their length (decode cost ~ samples), every rank hands its share to `runner` in calls of
    <= `batch` units; rank 0 returns every unit's text in table order (None elsewhere)."""
    costs = [float(b - a) for _, _, a, b in units]
    run = lambda g: pkg.shard.run_sharded(units, costs, None, rank, world, group=g, batch=max(batch, 2), batch_work=runner)
    return run(group) if (group is not None or world == 1) else _gloo_gather(run)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="voxtral-transcribe", description="Transcribe audio using Voxtral Mini 4B Realtime (MI355X HIP path)")
    ap.add_argument("-a", "--audio", action="append", default=[])
    ap.add_argument("--audio-list")
    ap.add_argument("-m", "--model", default="models/voxtral")
    ap.add_argument("--gguf")
    ap.add_argument("--tokenizer")
    ap.add_argument("-d", "--delay", type=int, default=6)
    ap.add_argument("--max-mel-frames", type=int, default=1200)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1, help="extension: shard the input files over N GPUs of this node (one process per GPU, longest-first "
                    "assignment, no collective in the data path; stdout keeps one line per input in input order)")
    ap.add_argument("--batch", type=int, default=1, help="extension: every file is split into its --max-mel-frames chunks and up to N chunks go into one "
                    "vox_transcribe_batch_ex call (continuous batching; same ids per chunk and the same lines as one by one; output order unchanged)")
    ap.add_argument("--sessions-per-gpu", type=int, default=1, help="extension (with --batch, Q4 GGUF): this many concurrent sessions on every GPU (own context + model replica + "
                    "library thread each: vox_model_set_sessions): one session's launch-bound decode steps leave gaps a second session fills (647 FLEURS-like clips: 3.7 s against 4.3 s; "
                    "calls with fewer than 128 units per session stay on one); same lines")
    ap.add_argument("--live", action="store_true", help="extension: feed every file through a live streaming session (vox_stream) in --live-chunk-ms pieces; the text so far "
                    "goes to stderr as ids arrive, stdout keeps one final line per input, equal to the un-chunked path's (Q4 GGUF, one GPU, no --batch)")
    ap.add_argument("--live-chunk-ms", type=int, default=160, help="with --live: milliseconds of audio per push (one decoder position = 160 ms)")
    ap.add_argument("--live-native-rate", action="store_true", help="with --live, for a file that is not at 16 kHz: push the file's own-rate samples into a session created "
                    "for that rate (it resamples as they arrive) instead of resampling the whole file first; the line is the same")
    ap.add_argument("--live-group", type=int, default=0, metavar="N", help="with --live: feed the files N (2..16) at a time through one stream group (vox_stream_group): every "
                    "weight matrix is read once per tick for all files that have a tick due; same final lines, in input order")
    ap.add_argument("--live-page-rows", type=int, default=None, metavar="R", help="with --live-group: a paged group (vox_stream_group_create_paged) whose decoder cache is one pool "
                    "of K / V pages of R rows (a power of two in 16..1024; 0: 256) that the files grow into, instead of a 2048-position slab slice per member; same lines")
    ap.add_argument("--live-pool-pages", type=int, default=None, metavar="P", help="with --live-group: a paged group with a pool of P pages (0: the default slab's memory)")
    ap.add_argument("--live-kv", choices=("f32", "bf16"), default=None, help="with --live-group: what the group's decoder K/V pool holds (vox_stream_group_create_kv; makes the "
                    "group a paged one).  bf16: 16-bit pages, half the memory per page and half the bytes the decode attention reads; the text may differ from an f32 group's "
                    "where the model's choice between two tokens is close")
    ap.add_argument("--live-delays", metavar="D,D,...", help="with --live-group: one delay per member (N values; a single value serves all), overriding --delay: the group is "
                    "made with a t_embed per member (vox_stream_group_create_t_embeds), member k's files run at the k-th delay, and every --live-words line gains the "
                    "member's delay")
    ap.add_argument("--live-burst", type=int, default=0, metavar="B", help="with --live: a burst stream (vox_stream_create_burst) -- a chunk that makes several ticks due (--live-chunk-ms "
                    "above 160) runs them in bursts of up to B (1..16): one encoder pass for the burst, then its decode steps")
    ap.add_argument("--live-endless", action="store_true", help="with --live: an endless session (vox_stream_create_endless) -- no limit at "
                    "16 384 decoder positions (about 43 minutes); the decoder cache is a ring of a little more than one window and stops growing there.  With --live-group: "
                    "an endless paged group (vox_stream_group_create_endless; --live-page-rows / --live-pool-pages apply), no member refused at 43 minutes; same lines")
    ap.add_argument("--live-suspend-every", type=int, default=0, metavar="N", help="with --live (also with --live-group): after every N pushes the session is snapshotted to "
                    "host memory, its stream freed (its member reset), and a fresh one restored from the blob; the output is unchanged")
    ap.add_argument("--live-peek", action="store_true", help="with --live (also with --live-group, --live-native-rate, --live-words): after every push a line starting with "
                    "'  ~[' on stderr: the text so far plus the tentative tail, i.e. the line if the file ended here (vox_stream_peek); stdout, the '  [' lines and the "
                    "words file do not change")
    ap.add_argument("--live-levels", action="store_true", help="with --live (also with --live-group): run the sessions with levels on (vox_stream_set_levels): every "
                    "--live-words line also carries peak_db and rms_db, the level of the audio the model had just heard while it chose the word's ids")
    ap.add_argument("--live-endpoint-ms", type=int, default=None, metavar="MS", help="with --live (implies --live-levels): the end-of-speech hint -- after a push whose quiet time "
                    "(trailing 160 ms ticks with a peak below --live-endpoint-db) has reached MS, peek once per quiet run and print the tentative \"  ~[\" line as "
                    "--live-peek prints it, then go on; the next non-quiet tick re-arms it")
    ap.add_argument("--live-endpoint-db", type=float, default=-50.0, metavar="DB", help="with --live-endpoint-ms: the quiet threshold in dBFS of the gained samples (default -50)")
    ap.add_argument("--live-words", metavar="PATH", help="with --live: run the sessions with scores on (vox_stream_set_scores) and write one JSON line per word to PATH when "
                    "a file ends: text, first_id / last_id (indices into the file's ids), due_s (when the session hands the word's last id out, in seconds of pushed audio: "
                    "not where the word was said), logprob (summed over the word's ids), min_margin (the smallest top-2 margin among them), file; stdout is unchanged")
    ap.add_argument("--live-alternatives", type=int, default=None, metavar="K", help="with --live-words: also keep every id's K (1..8) best alternatives and its step's entropy "
                    "(vox_stream_set_alternatives); every word line gains entropy (the largest over the word's ids) and weakest: {k: the index of its smallest-margin id, "
                    "alternatives: [{id, text, logprob}] of that id}; ids, stdout and the lines of runs without the flag are unchanged")
    ap.add_argument("--words", metavar="PATH", help="extension, without --live (one by one, --audio-list, --batch): every id comes with its score record "
                    "(vox_transcribe_batch_scored; one by one: vox_records_rows on the chunk's logits rows) and one JSON line per word goes to PATH: text, first_id / last_id "
                    "(indices into the ids of the file, or of the chunk for a file split by --max-mel-frames), logprob (summed over the word's ids), min_margin (the smallest "
                    "top-2 margin among them), file and, for a chunked file, chunk; stdout is unchanged")
    ap.add_argument("--alternatives", type=int, default=None, metavar="K", help="with --words: also every id's K (1..8) best alternatives and its step's entropy; every word "
                    "line gains entropy and weakest, as with --live-alternatives")
    a = ap.parse_args(argv)
    if a.alternatives is not None and not a.words:
        ap.error("--alternatives applies with --words")
    if a.alternatives is not None and not 1 <= a.alternatives <= 8:
        ap.error("--alternatives takes 1..8")
    if a.words and a.live:
        ap.error("--words serves the offline and batch paths: with --live use --live-words")
    if a.words and a.gpus > 1:
        ap.error("--words runs on one GPU (no --gpus): the ranks' records are not gathered")
    if a.live_alternatives is not None and not a.live_words:
        ap.error("--live-alternatives applies with --live-words")
    if a.live_alternatives is not None and not 1 <= a.live_alternatives <= 8:
        ap.error("--live-alternatives takes 1..8")
    a.live_alternatives = a.live_alternatives or 0
    if a.live_endpoint_ms is not None and (not a.live or a.live_endpoint_ms <= 0):
        ap.error("--live-endpoint-ms MS (MS > 0) applies with --live")
    if a.live_levels and not a.live:
        ap.error("--live-levels applies with --live")
    a.live_endpoint_ms = a.live_endpoint_ms or 0
    a.live_levels = a.live_levels or bool(a.live_endpoint_ms)
    if a.live_peek and not a.live:
        ap.error("--live-peek applies with --live")
    if a.live_suspend_every and (not a.live or a.live_suspend_every < 0):
        ap.error("--live-suspend-every N (N >= 1) applies with --live")
    if a.live_words and not a.live:
        ap.error("--live-words applies with --live")
    if a.live_group and not a.live:
        ap.error("--live-group applies with --live")
    if a.live_group and not 2 <= a.live_group <= 16:
        ap.error("--live-group takes 2..16 members")
    if (a.live_page_rows is not None or a.live_pool_pages is not None) and not a.live_group:
        ap.error("--live-page-rows / --live-pool-pages apply with --live-group")
    if a.live_kv is not None and not a.live_group:
        ap.error("--live-kv applies with --live-group")
    if a.live_delays is not None and not a.live_group:
        ap.error("--live-delays applies with --live-group")
    if a.live_delays is not None:
        try:
            a.live_delays = parse_live_delays(a.live_delays, a.live_group)
        except ValueError as e:
            ap.error(str(e))
    if a.live_page_rows not in (None, 0) and not (16 <= a.live_page_rows <= 1024 and a.live_page_rows & (a.live_page_rows - 1) == 0):
        ap.error("--live-page-rows takes a power of two in 16..1024 (0: 256)")
    if a.live_pool_pages is not None and a.live_pool_pages < 0:
        ap.error("--live-pool-pages takes a page count (0: the default)")
    if a.live_group and a.live_native_rate:
        ap.error("--live-group feeds 16 kHz samples: it does not combine with --live-native-rate")
    if a.live and (a.gpus > 1 or a.batch > 1 or a.live_chunk_ms <= 0):
        ap.error("--live runs one file at a time on one GPU (no --gpus / --batch) with --live-chunk-ms > 0")
    if a.live_endless and not a.live:
        ap.error("--live-endless applies with --live")
    if a.live_burst and (not a.live or a.live_group):
        ap.error("--live-burst applies with --live (a solo session; --live-group runs a plain group: burst groups are create_stream_group(burst=B))")
    if a.live_burst and not 1 <= a.live_burst <= 16:
        ap.error("--live-burst takes 1..16")
    if a.live_native_rate and not a.live:
        ap.error("--live-native-rate applies with --live")
    if a.live and not a.gguf:
        ap.error("--live needs a Q4 GGUF model (--gguf): live sessions do not serve the f32 SafeTensors path")
    if a.audio_list and a.audio:
        ap.error("--audio-list conflicts with --audio")
    if a.gguf and not a.tokenizer:
        ap.error("--gguf requires --tokenizer")
    paths = a.audio
    if a.audio_list:
        paths = [l.strip() for l in open(a.audio_list) if l.strip()]
    if not paths:
        ap.error("No audio files specified")
    if a.max_mel_frames <= 0:
        ap.error("--max-mel-frames must be greater than 0")
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package
    pkg = load_package()
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    if a.gpus > 1 and world == 1:
        # the reference transcribes its files one after the other (bin/transcribe.rs:112-126); here they are independent units of work for N replicas:
        # re-launch this command as N ranks (the driver's own launch for bench.py --gpus N); rank 0 prints every line, in input order
        n_dev = pkg.device_count()
        if n_dev < a.gpus:
            log(f"Error: --gpus {a.gpus} requested but {n_dev} GPU(s) visible"); return 2
        rc, out = pkg.shard.spawn_ranks(a.gpus, os.path.abspath(__file__), list(argv if argv is not None else sys.argv[1:]), capture=True)
        sys.stdout.write(out); sys.stdout.flush()
        return rc
    own_group = False
    if world > 1:
        a.device = int(os.environ.get("LOCAL_RANK", rank))
        if a.gguf:
            # torch BEFORE the first call into libvoxtral_hip.so (it bundles its own libamdhip64: one HIP runtime per process), then RCCL for the start-up broadcast
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(a.device)
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if not dist.is_initialized():
                dist.init_process_group(backend="nccl", device_id=torch.device("cuda", a.device)); own_group = True
    tok_path = a.tokenizer or os.path.join(a.model, "tekken.json")
    if not os.path.exists(tok_path):
        log(f"Error: Tokenizer not found at {tok_path}"); return 1
    tokenizer = pkg.VoxtralTokenizer.from_file(tok_path)
    ctx = pkg.Context(a.device)
    t0 = time.time()
    if a.gguf and world > 1:
        # N replicas: rank 0 reads the file, the packed weights reach the other GPUs with ONE RCCL broadcast over xGMI (shard.load_replicated) instead of N file reads
        st = {}
        log(f"[rank {rank}] Loading Q4 GGUF model from {a.gguf} ({'file' if rank == 0 else 'layout only + broadcast'})")
        model = pkg.shard.load_replicated(pkg, ctx, a.gguf, rank, world, local=a.device, stats=st)
        log(f"[rank {rank}] weight broadcast: {st.get('bytes', 0) / 1e9:.2f} GB in {st.get('seconds', 0.0):.3f}s")
    elif a.gguf:
        log(f"Loading Q4 GGUF model from {a.gguf}"); model = pkg.Q4ModelLoader.from_file(a.gguf).load(ctx)
    else:
        st = os.path.join(a.model, "consolidated.safetensors")
        log(f"Loading f32 model from {st}"); model = pkg.VoxtralModelLoader.from_file(st).load(ctx)
    log(f"Model loaded in {time.time() - t0:.2f}s")
    t_embed = pkg.TimeEmbedding(model.config.dec_dim).embed(float(a.delay))
    mel = pkg.MelSpectrogram.voxtral(ctx); pad_cfg = pkg.PadConfig.voxtral()
    chunk_cfg = pkg.ChunkConfig.voxtral().with_max_frames(a.max_mel_frames)
    rc = 0
    texts = {}
    words_out = open(a.live_words, "w", encoding="utf-8") if a.live_words else None
    rec_out = open(a.words, "w", encoding="utf-8") if a.words else None      # --words (never with --live: checked above)
    if a.batch > 1:
        # every file -> its chunks (transcribe.rs:210-226); ALL units of this rank's share go to vox_transcribe_batch_ex in calls of <= --batch units (continuous batching
        # over decode slots); a file's line = its chunk texts joined by " " (:261-275).  Files with a failed unit fall back to the one-by-one path below.
        units = unit_table(pkg, paths, chunk_cfg)
        if a.sessions_per_gpu > 1 and a.gguf:      # vox_model_set_sessions: calls with >= 128 units per session run as that many concurrent sessions on this GPU
            model.set_sessions(a.sessions_per_gpu)
            log(f"{a.sessions_per_gpu} sessions on this GPU (model replicated device to device)")
        n_units_of = {}
        for i, _, _, _ in units:
            n_units_of[i] = n_units_of.get(i, 0) + 1
        runner = UnitRunner(pkg, ctx, model, tokenizer, paths, t_embed, alts_k=(a.alternatives or 0) if rec_out is not None else None,
                            chunked=[i for i, c in n_units_of.items() if c > 1])
        try:
            unit_texts = sharded_units(pkg, units, runner, a.batch, rank, world) if units else []
        finally:
            if a.sessions_per_gpu > 1 and a.gguf:
                model.set_sessions(1)
        if unit_texts is not None:      # (rank 0, or the only rank)
            texts = join_units(len(paths), units, unit_texts)
            if rec_out is not None:      # the words of the files whose line stands, file-major; the others' come from the one-by-one path with their line
                for i, k, _, _ in units:
                    if i in texts:
                        write_word_lines(rec_out, runner.words.get((i, k), []))
    if a.live_group:
        try:
            texts = transcribe_live_group(pkg, paths, model, tokenizer, mel, t_embed, a.live_chunk_ms, a.live_group, words_out, a.live_peek, a.live_alternatives, a.live_page_rows, a.live_pool_pages, a.live_endless, a.live_suspend_every, a.live_kv, a.live_delays, a.live_levels, a.live_endpoint_ms, a.live_endpoint_db)
        except Exception as e:      # the files fall back to one live session each
            log(f"Error in the stream group: {e}"); texts = {}
            if words_out is not None:      # the files' words come again with their lines
                words_out.seek(0); words_out.truncate()
    def one(i):
        nonlocal rc
        if i in texts:
            return texts[i]
        p = paths[i]
        try:
            t1 = time.time()
            text = transcribe_live(pkg, p, model, tokenizer, mel, t_embed, a.live_chunk_ms, a.live_native_rate, words_out, a.live_peek, a.live_alternatives, a.live_endless, a.live_suspend_every, a.live_burst, a.live_levels, a.live_endpoint_ms, a.live_endpoint_db) if a.live else transcribe_one(pkg, p, model, tokenizer, mel, pad_cfg, chunk_cfg, t_embed, rec_out, a.alternatives or 0)
            log(f"{p}: {time.time() - t1:.3f}s")
        except Exception as e:      # per-utterance failure isolates to that line (empty), eval_wer.py:211-223 tolerates it
            log(f"Error transcribing {p}: {e}"); text = ""; rc = 1
        return text
    if world > 1 and a.batch > 1:
        if rank == 0:      # the units were sharded above; what is left (unreadable files, failed units) is rank 0's
            for i in range(len(paths)):
                print(one(i), flush=True)
    elif world > 1:
        lines = sharded_lines(pkg, paths, one, rank, world)
        if rank == 0:
            for text in lines:
                print(text, flush=True)
    else:
        for i in range(len(paths)):
            print(one(i), flush=True)
    if words_out is not None:
        words_out.close()
    if rec_out is not None:
        rec_out.close()
    if own_group:
        import torch.distributed as dist
        dist.barrier(); dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
