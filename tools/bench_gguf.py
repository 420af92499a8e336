"""GGUF dequantisation: rate per GGML type against a plain device copy of the same bytes, and the load time of a full-size synthetic Flux file.

    python tools/bench_gguf.py rates [--out profiles/gguf_dequant_rates.json]
    python tools/bench_gguf.py load  [--dir /tmp] [--blocks 19,38] [--out profiles/gguf_flux_q8_0_load.json]

rates: every supported type on a 3072 x 21504 tensor (Flux's widest matrix) of seeded random bytes, bf16 and fp16 output: median of 25 launches
after 5 warm-up launches, device events around each launch; in the same process, a `copy_` between two device buffers of (packed + 16-bit) / 2
bytes -- it reads and writes that many, so it moves the same number of bytes as the kernel.  `ratio` = copy time / kernel time (1.0: the kernel
streams as fast as a copy does).
load: writes a Flux.1-dev-shaped transformer (19 + 38 blocks, all matrices Q8_0, vectors F32: ~12.7 GB) of random blocks with tools/gguf_write.py,
then times forge_loader's parts on it: parsing + mapping, the host's read of the packed bytes into the pinned staging buffer, the host-to-device
copies, the dequantisation kernels (device events), and the whole forge_loader call (wall clock, ends in a device synchronise)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import forge_amd  # noqa: E402,F401
from forge_amd import _lib, hipops as ops, synth  # noqa: E402
from forge_amd.backend import loader  # noqa: E402
from forge_amd.backend.gguf_file import DEQUANT_TYPES, GGML_TYPES  # noqa: E402
from gguf_write import write_gguf  # noqa: E402

ROWS, COLS = 3072, 21504


def _timed(fn, warmup=5, reps=25):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def rates(out_path):
    n = ROWS * COLS
    rng = np.random.default_rng(0)
    rows = []
    for qt in DEQUANT_TYPES:
        name, bw, bb = GGML_TYPES[qt]
        packed = n // bw * bb
        raw = torch.from_numpy(rng.integers(0, 256, packed, dtype=np.uint8)).cuda()
        moved = packed + 2 * n
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy_ms = _timed(lambda: dst.copy_(src))
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
            out = torch.empty((ROWS, COLS), dtype=dt, device="cuda")
            k_ms = _timed(lambda: ops.gguf_dequant(raw, qt, (ROWS, COLS), dt, out=out))
            rows.append(dict(type=name, out=tag, bytes_in=packed, bytes_out=2 * n, kernel_ms_median=round(k_ms[0], 4), kernel_ms_min=round(k_ms[1], 4),
                             kernel_ms_max=round(k_ms[2], 4), kernel_TBps=round(moved / k_ms[0] * 1e-9, 3), copy_ms_median=round(copy_ms[0], 4),
                             copy_TBps=round(moved / copy_ms[0] * 1e-9, 3), ratio=round(copy_ms[0] / k_ms[0], 3)))
            print(json.dumps(rows[-1]), flush=True)
        del raw, src, dst
    res = dict(shape=[ROWS, COLS], launches=25, warmup=5, device=torch.cuda.get_device_name(0), library=_lib.build_info(), rows=rows)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    return res


def synth_flux_q8_0(path, depth, depth_single):
    from forge_amd.backend.nn.layout import flux_param_shapes
    cfg = dict(synth.FLUX_DEV_CONFIG, depth=depth, depth_single_blocks=depth_single)
    rng = np.random.default_rng(1)
    pool = {}
    tensors = []
    for name, shape in flux_param_shapes(cfg).items():
        n = int(np.prod(shape))
        if len(shape) < 2 or shape[-1] % 32:
            tensors.append((name, 0, tuple(shape), np.zeros(n, dtype=np.float32).view(np.uint8)))
            continue
        if n not in pool:                       # one buffer of random blocks per tensor size: the file's content does not matter, its size does
            blk = rng.integers(0, 256, (n // 32, 34), dtype=np.uint8)
            blk[:, 1] &= 0x3F                   # finite, small fp16 scales
            pool[n] = blk.reshape(-1)
        tensors.append((name, 8, tuple(shape), pool[n]))
    write_gguf(path, tensors, {"general.architecture": "flux"})
    return cfg, os.path.getsize(path)


def load(directory, depth, depth_single, out_path, keep=False):
    path = os.path.join(directory, "synthetic_flux_q8_0.gguf")
    t0 = time.perf_counter()
    cfg, size = synth_flux_q8_0(path, depth, depth_single)
    write_s = time.perf_counter() - t0
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sd = loader.load_torch_file(path)
        parse_s = time.perf_counter() - t0
        quant = [v for v in sd.values() if v.qtype == 8]
        cap = max(v.data.nbytes for v in quant)
        pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
        dev = torch.empty(cap, dtype=torch.uint8, device="cuda")
        out = torch.empty(max(v.numel for v in quant), dtype=torch.bfloat16, device="cuda")
        read_s = h2d_ms = kern_ms = 0.0
        for v in quant:                          # the three parts one after the other, each on its own clock
            n = v.data.nbytes
            t1 = time.perf_counter()
            pinned[:n].numpy()[:] = v.data
            read_s += time.perf_counter() - t1
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            dev[:n].copy_(pinned[:n], non_blocking=True)
            b.record()
            ops.gguf_dequant(dev[:n], 8, (v.numel,), torch.bfloat16, out=out[:v.numel])
            c.record()
            c.synchronize()
            h2d_ms += a.elapsed_time(b)
            kern_ms += b.elapsed_time(c)
        del pinned, dev, out, sd
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = loader.forge_loader(path, device="cuda")
        torch.cuda.synchronize()
        total_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        eng2 = loader.forge_loader(path, device="cuda")      # second call: the file is in the page cache
        torch.cuda.synchronize()
        total2_s = time.perf_counter() - t0
        del eng, eng2
    finally:
        if not keep:
            os.remove(path)
    res = dict(file_bytes=size, depth=[depth, depth_single], write_s=round(write_s, 2), parse_and_map_s=round(parse_s, 4), tensors_q8_0=len(quant),
               host_read_into_pinned_s=round(read_s, 3), host_to_device_s=round(h2d_ms * 1e-3, 3), dequant_kernels_s=round(kern_ms * 1e-3, 4),
               forge_loader_wall_s=round(total_s, 3), forge_loader_wall_second_call_s=round(total2_s, 3), device=torch.cuda.get_device_name(0),
               library=_lib.build_info())
    print(json.dumps(res), flush=True)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["rates", "load"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--blocks", default="19,38")
    ap.add_argument("--keep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gguf.py measures on the GPU: no device found")
    if a.mode == "rates":
        rates(a.out)
    else:
        d, s = (int(x) for x in a.blocks.split(","))
        load(a.dir, d, s, a.out, a.keep)
