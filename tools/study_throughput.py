#!/usr/bin/env python3
"""Row f3 as a measurement: studies per second through process_folder (reference calculate_optical_flow.py:243-290) on the
GPU box, HDF5 writing included, with the writer thread beside the next solve and without it.  h5py lives in the image's
second interpreter, so run it there:
    LD_PRELOAD=/usr/lib/x86_64-linux-gnu/libstdc++.so.6 /opt/conda/bin/python3.9 tools/study_throughput.py [--studies 6] [--frames 65] [--size 512]
--payload host|device: who makes the file's float16 `flow` and `echo` (process_folder(payload=)).  --compare-payloads R: only the
worker-process walk, R rounds for each payload, interleaved in one process (same box, same folder), with the caller's thread's times.
--deflate host|device: who compresses `flow` and `echo` (process_folder(deflate=), needs --payload device).  --compare-deflates R: the
same form for deflate host and device under payload="device": R rounds each, interleaved, then the medians, the round-by-round
differences, the host's zlib.compress calls per study (counted from the chunks of the files each walk wrote: every chunk of a dataset
create_gzip9 hands over itself, less those the device made), study_download_bytes per study and the device time of deflate's match
search and parse per study (the engine's counters).  --height / --width: frames that are not square."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--studies", type=int, default=6)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--algo", default="TVL1")
    ap.add_argument("--readers", type=int, default=2)
    ap.add_argument("--writers", type=int, default=2)
    ap.add_argument("--stages", action="store_true", help="also print where the caller's thread spends a study in the worker-process walk")
    ap.add_argument("--payload", choices=("host", "device"), default="host", help="process_folder(payload=): who casts flow and echo to float16")
    ap.add_argument("--compare-payloads", type=int, default=0, metavar="R",
                    help="R rounds of the worker-process walk for payload host and device, interleaved; nothing else is run")
    ap.add_argument("--deflate", choices=("host", "device"), default="host", help="process_folder(deflate=): who compresses flow and echo")
    ap.add_argument("--compare-deflates", type=int, default=0, metavar="R",
                    help="R rounds of the worker-process walk for deflate host and device (payload device), interleaved; nothing else is run")
    ap.add_argument("--height", type=int, default=0, help="frame height (default: --size)")
    ap.add_argument("--width", type=int, default=0, help="frame width (default: --size)")
    a = ap.parse_args()
    if a.compare_deflates > 0:
        a.payload = "device"
    if a.deflate == "device" and a.payload != "device":
        ap.error("--deflate device needs --payload device")
    H, W = a.height or a.size, a.width or a.size
    from tee_optical_flow_amd import pipeline as P
    from tee_optical_flow_amd import hdf5_out
    from tee_optical_flow_amd.synth import speckle_sequence
    tmp = tempfile.mkdtemp(prefix="teeflow_studies_")
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    for k in range(a.studies):
        g = speckle_sequence(500 + k, a.frames, H, W)
        np.savez(os.path.join(src, f"study{k:02d}.npz"), nparr=np.repeat(g[..., None], 3, axis=3), pixel_spacing=0.04, frame_rate=50.0, patient_id=f"S{k}")
    # the worker processes must exist before anything in this process touches the GPU
    workers = P.StudyWorkers(a.readers, a.writers)
    model = P.make_flow_model(a.algo)
    kw = dict(nchunks=1, chunk_index=0, mode="otsu", verbose=False, extensions=("npz",), OF_algo=a.algo, flow_model=model, payload=a.payload,
              deflate=a.deflate)
    P.process_folder(src, os.path.join(tmp, "warm"), None, process_subset=True, file_subset_list=["study00.npz"], workers="thread", **kw)   # warm-up: allocations, masks code paths
    P.process_folder(src, os.path.join(tmp, "warm2"), None, process_subset=True, file_subset_list=["study00.npz", "study01.npz"], workers=workers, **kw)
    # where the caller's thread spends a study in the worker-process walk: solve (flow_for_study), hand-over to the writer (defer),
    # the rest of process_video, and everything outside it (waiting for the reader stage, reaping writers)
    acc = {"begin": 0.0, "finish": 0.0, "defer": 0.0}
    real_begin = P._process_video_begin

    def timed_begin(*args, **kwargs):
        d = kwargs.get("_defer_save")
        if d is not None:
            def timed_defer(job, *more):
                t = time.perf_counter(); d(job, *more); acc["defer"] += time.perf_counter() - t
            kwargs["_defer_save"] = timed_defer
        t = time.perf_counter()
        fin = real_begin(*args, **kwargs)                   # masks are ready; conditions the frames and SUBMITS the solve (studies_in_flight=2)
        acc["begin"] += time.perf_counter() - t

        def timed_finish():
            t2 = time.perf_counter()
            try:
                return fin()                                # waits for the flows, hands the study to the writer stage
            finally:
                acc["finish"] += time.perf_counter() - t2
        return timed_finish
    if a.compare_payloads > 0:
        # flows of N - 1 pairs (the last one is repeated on the host), float32 or float16; device payload: plus the echo's N frames of halves
        px = H * W
        d2h = {"host": (a.frames - 1) * px * 2 * 4, "device": (a.frames - 1) * px * 2 * 2 + a.frames * px * 2}
        P._process_video_begin = timed_begin
        print(f"{a.algo}: {a.studies} studies of {a.frames} frames {H}x{W}, {a.readers} reader + {a.writers} writer processes, Otsu masks")
        for payload in ("host", "device"):                  # one more warm-up each: the payload's own buffers (pinned pool, staging, echo)
            P.process_folder(src, os.path.join(tmp, f"warm_{payload}"), None, process_subset=True, file_subset_list=["study00.npz", "study01.npz"],
                             workers=workers, **{**kw, "payload": payload})
        for r in range(a.compare_payloads):
            for payload in ("host", "device"):
                acc.update(begin=0.0, finish=0.0, defer=0.0)
                t0 = time.perf_counter()
                errs = P.process_folder(src, os.path.join(tmp, f"cmp_{payload}{r}"), None, workers=workers, **{**kw, "payload": payload})
                t = time.perf_counter() - t0
                n = a.studies
                print(f"  round {r} payload={payload:6s}: {t / n * 1e3:7.1f} ms per study; caller's thread per study: submit {acc['begin'] / n * 1e3:6.1f} ms, "
                      f"collect + hand-over {acc['finish'] / n * 1e3:6.1f} ms (hand-over to the writer {acc['defer'] / n * 1e3:6.1f} ms); "
                      f"D2H {d2h[payload] / 1e6:.1f} MB per study (errors: {errs})", flush=True)
                shutil.rmtree(os.path.join(tmp, f"cmp_{payload}{r}"), ignore_errors=True)
        P._process_video_begin = real_begin
        workers.close()
        model.close()
        shutil.rmtree(tmp, ignore_errors=True)
        return
    if a.compare_deflates > 0:
        import h5py

        def host_zlib_calls(folder, deflate):
            """zlib.compress calls of the writer stage per study, from the files: create_gzip9 compresses every chunk of a dataset
            of min_parallel_bytes or more itself, unless the device made its record (flow and echo under deflate="device")"""
            n = 0
            for f in os.listdir(folder):
                with h5py.File(os.path.join(folder, f), "r") as h:
                    n += sum(h[k].id.get_num_chunks() for k in h if h[k].nbytes >= hdf5_out.MIN_PARALLEL_BYTES and not (deflate == "device" and k in ("flow", "echo")))
            return n / a.studies
        P._process_video_begin = timed_begin
        print(f"{a.algo}: {a.studies} studies of {a.frames} frames {H}x{W}, {a.readers} reader + {a.writers} writer processes, Otsu masks, payload=device")
        for deflate in ("host", "device"):                  # one more warm-up each: deflate's own device buffers
            P.process_folder(src, os.path.join(tmp, f"warm_{deflate}"), None, process_subset=True, file_subset_list=["study00.npz", "study01.npz"],
                             workers=workers, **{**kw, "deflate": deflate})
        ms = {"host": [], "device": []}
        names = ("study_download_bytes", "deflate_match_us", "deflate_emit_us")
        for r in range(a.compare_deflates):
            for deflate in ("host", "device"):
                acc.update(begin=0.0, finish=0.0, defer=0.0)
                c0 = {k: model.counter(k) for k in names}
                dst = os.path.join(tmp, f"cmp_{deflate}{r}")
                t0 = time.perf_counter()
                errs = P.process_folder(src, dst, None, workers=workers, **{**kw, "deflate": deflate})
                t = time.perf_counter() - t0
                n = a.studies
                c = {k: (model.counter(k) - c0[k]) / n for k in names}
                ms[deflate].append(t / n * 1e3)
                print(f"  round {r} deflate={deflate:6s}: {t / n * 1e3:7.1f} ms per study; caller's thread per study: begin {acc['begin'] / n * 1e3:6.1f} ms, "
                      f"finish {acc['finish'] / n * 1e3:6.1f} ms (hand-over to the writer {acc['defer'] / n * 1e3:6.1f} ms); host zlib.compress calls "
                      f"{host_zlib_calls(dst, deflate):.0f} per study; study_download_bytes {c['study_download_bytes'] / 1e6:.1f} MB per study; device "
                      f"match search {c['deflate_match_us'] / 1e3:.1f} ms + parse {c['deflate_emit_us'] / 1e3:.1f} ms per study (errors: {errs})", flush=True)
                shutil.rmtree(dst, ignore_errors=True)
        diff = [d - h for h, d in zip(ms["host"], ms["device"])]
        print(f"  median ms per study: host {np.median(ms['host']):.1f}, device {np.median(ms['device']):.1f}; device - host by round: "
              + ", ".join(f"{d:+.1f}" for d in diff) + f" ms ({', '.join(f'{100 * d / h:+.1f} %' for h, d in zip(ms['host'], diff))})")
        P._process_video_begin = real_begin
        workers.close()
        model.close()
        shutil.rmtree(tmp, ignore_errors=True)
        return
    if a.stages:
        P._process_video_begin = timed_begin
    t0 = time.perf_counter()
    errs_p = P.process_folder(src, os.path.join(tmp, "processes"), None, workers=workers, **kw)
    t_proc = time.perf_counter() - t0
    P._process_video_begin = real_begin
    if a.stages:
        n = a.studies
        print(f"  caller's thread per study (worker-process walk, the next study's solve submitted before this one's is collected): submit (conditioning "
              f"+ queueing) {acc['begin'] / n * 1e3:.1f} ms, collect + hand-over {acc['finish'] / n * 1e3:.1f} ms (of which hand-over to the writer {acc['defer'] / n * 1e3:.1f} ms), "
              f"outside both (reader wait, reaping) {(t_proc - acc['begin'] - acc['finish']) / n * 1e3:.1f} ms")
    workers.close()
    t0 = time.perf_counter()
    errs = P.process_folder(src, os.path.join(tmp, "overlapped"), None, workers="thread", **kw)
    t_overlap = time.perf_counter() - t0
    # the same walk with the HDF5 write done in line (what the reference does): time the writer by making defer synchronous
    real = hdf5_out.save_optical_flow_to_hdf5
    t_write = [0.0]

    def timed(*args, **kwargs):
        t = time.perf_counter(); real(*args, **kwargs); t_write[0] += time.perf_counter() - t
    hdf5_out.save_optical_flow_to_hdf5 = timed
    orig_pf = P.process_folder

    def serial_folder(*args, **kwargs):
        # no writer thread: process_video writes before it returns
        files = sorted(os.listdir(args[0]))
        os.makedirs(args[1], exist_ok=True)
        for f in files:
            nparr, md, pid, hr = P.read_study(os.path.join(args[0], f))
            P.process_video(None, os.path.join(args[1], f[:-4] + ".hdf5"), None, verbose=False, mode="otsu", no_saliency=True, OF_algo=a.algo,
                            nparr=nparr, metadata=md, patient_id=pid, heart_rate=hr, flow_model=model, payload=a.payload, deflate=a.deflate)
    t0 = time.perf_counter()
    serial_folder(src, os.path.join(tmp, "serial"))
    t_serial = time.perf_counter() - t0
    hdf5_out.save_optical_flow_to_hdf5 = real
    model.close()
    sz = sum(os.path.getsize(os.path.join(tmp, "overlapped", f)) for f in os.listdir(os.path.join(tmp, "overlapped"))) / a.studies / 1e6
    print(f"{a.algo}: {a.studies} studies of {a.frames} frames {H}x{W} (errors: {errs})")
    print(f"  {a.readers} reader + {a.writers} writer PROCESSES      : {t_proc:6.2f} s = {t_proc / a.studies * 1e3:7.1f} ms per study, {a.studies * (a.frames - 1) / t_proc:7.1f} pairs/s end to end (errors: {errs_p})")
    print(f"  reader / writer threads            : {t_overlap:6.2f} s = {t_overlap / a.studies * 1e3:7.1f} ms per study, {a.studies * (a.frames - 1) / t_overlap:7.1f} pairs/s end to end")
    print(f"  write in line (reference order)    : {t_serial:6.2f} s = {t_serial / a.studies * 1e3:7.1f} ms per study, of which HDF5 gzip-9 write {t_write[0] / a.studies * 1e3:7.1f} ms; file {sz:.1f} MB per study")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
