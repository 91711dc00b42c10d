"""Where a k_gemm_ws launch spends its time, per block and per row tile: loads the stamp-instrumented
diagnostic library (make -C replicatinggpt_amd/csrc wsstamps; gemm_ws.hip CG_WS_STAMPS) and prints, for the
three weight-stationary products of the training census (bench.census_op: the step's epilogues), medians
over the launch's working blocks of
  prologue   start -> weights in registers and tiles 0 / 1 requested
  head       previous tile's stores issued -> this tile's counted wait and barrier passed (tile 0: from the
             prologue's end), per tile
  mfma       -> the tile's MFMA chain (and the tile after next's DMA issue) done, per tile
  epilogue   -> the tile's stores issued, per tile
  tail       last stores issued -> they have all left (the block's end)
  block      start -> end; launch = first start -> last end over all blocks
and, for the CUs that held two blocks, how far apart the two ran: the difference of their start stamps and of
their "head passed" stamps at the middle tile, the latter also as a fraction of the tile period (0 = in step,
0.5 = one block's MFMA chain under the other's epilogue).  Times are s_memrealtime ticks (100 MHz) in us,
taken by wave 0 of each block.  A timing instrument for a healthy kernel.  GPU only.
usage: python tools/ws_stamps.py [c2|c4]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["CHARPT_LIB"] = os.path.join(ROOT, "replicatinggpt_amd", "libcharpt_hip_wsstamps.so")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from replicatinggpt_amd import PRESETS  # noqa: E402
from replicatinggpt_amd import _lib as L  # noqa: E402

PRODUCTS = ("qkv_fwd", "ffn1_fwd", "ffn2_dgrad")
US = 0.01   # one s_memrealtime tick


def med(xs):
    xs = list(xs)
    return statistics.median(xs) if xs else float("nan")


def blocks_of(buf, words, nblocks):
    """the working blocks' records: dicts of start, weights, end, where, per-tile (head, mfma, stores)"""
    out = []
    for b in range(nblocks):
        w = buf[b * words:(b + 1) * words]
        ntile = int(w[4])
        if ntile == 0:
            continue
        rec = min(ntile, (words - 8) // 3)
        out.append({"start": w[0], "weights": w[1], "end": w[2], "where": (w[3] >> 32, (w[3] >> 8) & 0xff),
                    "ntile": ntile, "tiles": [tuple(w[8 + 3 * t:11 + 3 * t]) for t in range(rec)]})
    return out


def report(tag, us_event, blocks):
    head, mfma, epi = [], [], []
    for b in blocks:
        prev = b["weights"]
        for h, m, s in b["tiles"]:
            head.append((h - prev) * US)
            mfma.append((m - h) * US)
            epi.append((s - m) * US)
            prev = s
    head0 = [(b["tiles"][0][0] - b["weights"]) * US for b in blocks]
    launch = (max(b["end"] for b in blocks) - min(b["start"] for b in blocks)) * US
    per_tile = med(head) + med(mfma) + med(epi)
    print(f"{tag}: {us_event:6.1f} us by events, {launch:6.1f} us first start -> last end; {len(blocks)} working blocks, "
          f"{min(b['ntile'] for b in blocks)}..{max(b['ntile'] for b in blocks)} tiles each")
    print(f"    prologue {med((b['weights'] - b['start']) * US for b in blocks):5.2f}  tile-0 head {med(head0):5.2f}  | per tile: "
          f"head {med(head):5.2f}  mfma {med(mfma):5.2f}  epilogue {med(epi):5.2f}  (sum {per_tile:5.2f})  | "
          f"tail {med((b['end'] - b['tiles'][-1][2]) * US for b in blocks if len(b['tiles']) == b['ntile']):5.2f}  "
          f"block {med((b['end'] - b['start']) * US for b in blocks):6.2f}  start spread "
          f"{(max(b['start'] for b in blocks) - min(b['start'] for b in blocks)) * US:5.2f}")
    by_cu = {}
    for b in blocks:
        by_cu.setdefault(b["where"], []).append(b)
    pairs = [v for v in by_cu.values() if len(v) == 2]
    if pairs:
        dstart = [abs(a["start"] - b["start"]) * US for a, b in pairs]
        mid = [(a["tiles"][t][0] - b["tiles"][t][0]) * US for a, b in pairs
               for t in [min(len(a["tiles"]), len(b["tiles"])) // 2]]
        frac = [abs((d / per_tile + 0.5) % 1.0 - 0.5) for d in mid] if per_tile > 0 else []
        print(f"    {len(pairs)} CUs with two blocks ({len(by_cu)} CUs in all): starts {med(dstart):5.2f} us apart, "
              f"middle-tile heads {med(abs(d) for d in mid):5.2f} us apart = {med(frac):4.2f} of a tile period")
    else:
        print(f"    no CU held two blocks ({len(by_cu)} CUs in all)")


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
    lib = L.load()
    lib.cg_debug_ws_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    words = int(lib.cg_debug_ws_stamps_words())
    c = PRESETS[cfg]
    nblocks = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    buf = (ctypes.c_ulonglong * (nblocks * words))()
    for name, m, n, k, at, bt, kind, _ in bench.census_shapes(c, c.batch_size, c.block_size):
        if name not in PRODUCTS:
            continue
        fn, _ = bench.census_op(name, m, n, k, at, bt, kind, torch.device("cuda"))
        n0 = int(lib.cg_gemm_ws_launches())
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        assert int(lib.cg_gemm_ws_launches()) == n0 + 3, "k_gemm_ws did not take the product"
        assert lib.cg_debug_ws_stamps_reset() == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        assert lib.cg_debug_ws_stamps(ctypes.addressof(buf), nblocks) == 0
        report(f"{cfg} {name:10s} M={m} N={n} K={k}", a.elapsed_time(b) * 1e3, blocks_of(list(buf), words, nblocks))


if __name__ == "__main__":
    main()
