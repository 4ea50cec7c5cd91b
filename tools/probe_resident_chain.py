"""tools/probe_resident_chain.py [--size 30000] [--form both|numpy|resident] [--reps 5] [--out FILE] [--label TEXT]

The chain
    upstream_area("cell") -> upa > t -> stream_order(mask) -> hand(drain = strord >= s, elevtn)
on a synthetic SIZE x SIZE raster and elevation made on the device (``_hip.synth_*_device``), once through numpy arrays
(every link downloads its result and uploads it again for the next call: today's API, nothing else) and once resident
(``resident=True`` and ``DeviceArray`` expressions: only the final HAND is downloaded).  Per link and in total: host wall
time of calls that return with their result complete (every call of the library synchronises before it returns), the
library's own transfer clocks (``_hip.transfer_stats``), and for the elementwise kernels the GB/s of the bytes they must
move.  The release of a pass's arrays (host arrays; ``free()`` of the device arrays) is timed as links of its own, and a
pass's total is the sum of its links.  Transfers are read from both accounts: ``_hip.transfer_stats`` (staging copies inside
the library's calls) and ``_hip.buffer_transfer_stats`` (``to_device`` / ``.numpy()``).  ``--hipmalloc`` runs the resident
form with a ``hipMalloc`` behind every new ``DeviceArray``.  One warm-up pass, then ``--reps`` timed passes; the median,
the minimum and the maximum are reported.

The measurement runs in a child process under ``timeout`` (``--timeout`` seconds), which reserves its arena first, as
bench.py does.  ``--form numpy`` runs on a checkout that has no DeviceArray (the parent commit): ``--package-root`` names
the tree whose ``pyflwdir_amd`` is imported.  The report is appended to ``--out``.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
UPA_MIN, STO_MIN = 1000, 3  # t and s of the chain


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=30000)
    ap.add_argument("--form", choices=["both", "numpy", "resident"], default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reserve-gib", type=float, default=64.0)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--package-root", default=os.path.dirname(HERE))
    ap.add_argument("--hipmalloc", action="store_true",
                    help="resident form with DeviceArray buffers from pfd_malloc (hipMalloc) instead of the caching allocator")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


class Clock:
    """Wall time per named link over the passes; the first pass is the warm-up and is dropped."""

    def __init__(self):
        self.t, self.order = {}, []

    def link(self, name, fn):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        if name not in self.t:
            self.t[name] = []
            self.order.append(name)
        self.t[name].append(dt * 1e3)
        return r

    def lines(self, extra=None):
        out = []
        for name in self.order:
            v = self.t[name][1:]
            line = f"    {name:<34} median {statistics.median(v):9.2f} ms   min {min(v):9.2f}   max {max(v):9.2f}"
            if extra and name in extra:
                line += f"   {extra[name] / (statistics.median(v) * 1e-3) / 1e9:8.1f} GB/s ({extra[name] / 1e9:.2f} GB moved)"
            out.append(line)
        return out

    def sum_of_medians(self):
        return sum(statistics.median(self.t[name][1:]) for name in self.order)


def fmt_stats(st, passes):
    return (f"h2d {st['h2d_bytes'] / passes / 1e9:.3f} GB in {st['h2d_ms'] / passes:.1f} ms, d2h {st['d2h_bytes'] / passes / 1e9:.3f} GB "
            f"in {st['d2h_ms'] / passes:.1f} ms, prefault {st['prefault_ms'] / passes:.1f} ms, {st['host_results'] / passes:.0f} host results")


def measure(args):
    sys.path.insert(0, args.package_root)
    import numpy as np

    import pyflwdir_amd as pyflwdir
    from pyflwdir_amd import _hip

    size, n = args.size, args.size * args.size
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"== resident chain probe{' — ' + args.label if args.label else ''}: {size} x {size} = {n / 1e9:.2f} Gcells, "
        f"{args.reps} timed passes after 1 warm-up, t = {UPA_MIN}, s = {STO_MIN}")
    _hip.reserve(int(args.reserve_gib * 2**30), 0)  # the arena first, as bench.py does
    d8_buf = _hip.synth_d8_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
    elev_buf = _hip.synth_elev_device(size, size, seed=0, tilt=1 << 26, white=2, nodata_pct=0)
    d8 = d8_buf.download(np.uint8, (size, size))
    elevtn = elev_buf.download(np.float32, (size, size))
    d8_buf.free()
    flw = pyflwdir.from_array(d8, ftype="d8", cache=False)
    say(f"   raster: {flw._h.info(counts=True)['n_pits']} pits, device {_hip.mem_info(0)}")
    digest = {}

    buffer_stats = getattr(_hip, "buffer_transfer_stats", None)  # (a checkout before DeviceArray has no such account)

    def both_accounts(reset):
        """All host <-> device traffic since the last reset: the staging copies inside the library's calls
        (pfd_transfer_stats) and the copies of DeviceBuffer.upload / download, which DeviceArray's to_device / .numpy() are."""
        return _hip.transfer_stats(reset=reset), (buffer_stats(reset=reset) if buffer_stats else None)

    def fmt_both(st, sb, passes):
        out = f"inside the library's calls: {fmt_stats(st, passes)}"
        if sb is not None:
            out += (f"; DeviceArray's own copies: h2d {sb['h2d_bytes'] / passes / 1e9:.3f} GB in {sb['h2d_copies'] / passes:.0f} copies, "
                    f"d2h {sb['d2h_bytes'] / passes / 1e9:.3f} GB in {sb['d2h_copies'] / passes:.0f} copies ({sb['d2h_ms'] / passes:.1f} ms)")
        return out

    def total_line(total):
        return f"    {'TOTAL (links + releases)':<34} median {statistics.median(total[1:]):9.2f} ms   min {min(total[1:]):9.2f}   max {max(total[1:]):9.2f}"

    if args.form in ("both", "numpy"):
        clock, total = Clock(), []
        for p in range(args.reps + 1):
            if p == 1:
                both_accounts(True)
            t0 = time.perf_counter()
            upa = clock.link("upstream_area('cell')", lambda: flw.upstream_area("cell"))
            mask = clock.link("upa > t (numpy)", lambda: upa > UPA_MIN)
            sto = clock.link("stream_order(mask)", lambda: flw.stream_order(mask=mask))
            drain = clock.link("strord >= s (numpy)", lambda: sto >= STO_MIN)
            hand = clock.link("hand(drain, elevtn)", lambda: flw.hand(drain, elevtn))
            t1 = time.perf_counter()
            if p == args.reps:
                digest["numpy"] = (int(np.count_nonzero(drain)), float(hand.max()), hand[::997, ::991].tobytes())
            t2 = time.perf_counter()
            del upa, mask, sto, drain, hand  # (13.5 GB of host arrays at 30000^2: a user's loop pays this as well)
            t3 = time.perf_counter()
            clock.link("release of the 5 host arrays", lambda: None)
            clock.t["release of the 5 host arrays"][-1] = (t3 - t2) * 1e3
            total.append((t1 - t0 + t3 - t2) * 1e3)
        st, sb = both_accounts(True)
        say("  numpy form (today's API: every link goes through host arrays)")
        for s_ in clock.lines():
            say(s_)
        say(total_line(total))
        say(f"    transfers per pass — {fmt_both(st, sb, args.reps)}")

    if args.form in ("both", "resident"):
        from pyflwdir_amd import DeviceArray, device_array

        if args.hipmalloc:
            device_array.POOLED = False
            say("  (--hipmalloc: every new DeviceArray takes a hipMalloc of its own instead of a block of the caching allocator)")
        elev_dev = DeviceArray(elev_buf, (size, size), np.float32)
        clock, total = Clock(), []
        before = None
        for p in range(args.reps + 1):
            if p == 1:
                both_accounts(True)
                before = [dict.fromkeys(("h2d_bytes", "d2h_bytes", "host_results"), 0.0), dict.fromkeys(("h2d_bytes", "d2h_bytes"), 0)]
            t0 = time.perf_counter()
            st0, sb0 = both_accounts(False)
            upa = clock.link("upstream_area('cell', resident)", lambda: flw.upstream_area("cell", resident=True))
            mask = clock.link("upa > t (kernel)", lambda: upa > UPA_MIN)
            sto = clock.link("stream_order(mask, resident)", lambda: flw.stream_order(mask=mask, resident=True))
            drain = clock.link("strord >= s (kernel)", lambda: sto >= STO_MIN)
            hand_dev = clock.link("hand(drain, elevtn, resident)", lambda: flw.hand(drain, elev_dev, resident=True))
            st1, sb1 = both_accounts(False)
            if before is not None:  # what crossed between the start of the chain and its last link, summed over the timed passes
                for k in before[0]:
                    before[0][k] += st1[k] - st0[k]
                for k in before[1]:
                    before[1][k] += sb1[k] - sb0[k]
            hand = clock.link("hand.numpy() (the one download)", lambda: hand_dev.numpy())
            t1 = time.perf_counter()
            if p == args.reps:
                digest["resident"] = (drain.count_nonzero(), float(hand.max()), hand[::997, ::991].tobytes())
            t2 = time.perf_counter()
            for a in (upa, mask, sto, drain, hand_dev):
                a.free()
            t3 = time.perf_counter()
            del hand  # (the 7.2 GB host array of the result at 30000^2)
            t4 = time.perf_counter()
            for name, dt in (("free() of the 5 device arrays", t3 - t2), ("release of the host HAND array", t4 - t3)):
                clock.link(name, lambda: None)
                clock.t[name][-1] = dt * 1e3
            total.append((t1 - t0 + t4 - t2) * 1e3)
        st, sb = both_accounts(True)
        say("  resident form (DeviceArray between the links; only the final HAND is downloaded)")
        for s_ in clock.lines({"upa > t (kernel)": 5.0 * n, "strord >= s (kernel)": 2.0 * n}):
            say(s_)
        say(total_line(total))
        say(f"    transfers per pass, download included — {fmt_both(st, sb, args.reps)}")
        say(f"    transfers per pass between the start of the chain and the end of its last link (both accounts): inside the library's "
            f"calls h2d {before[0]['h2d_bytes'] / args.reps:.0f} bytes, d2h {before[0]['d2h_bytes'] / args.reps:.0f} bytes, "
            f"{before[0]['host_results'] / args.reps:.0f} host results; DeviceArray's own copies h2d {before[1]['h2d_bytes'] / args.reps:.0f} bytes, "
            f"d2h {before[1]['d2h_bytes'] / args.reps:.0f} bytes")
        # the other elementwise kernels at this size, each with the bytes it must move (reads + writes)
        upa = flw.upstream_area("cell", resident=True)
        mask = upa > UPA_MIN
        from pyflwdir_amd.device_array import where

        ew = Clock()
        kernels = {"int32 > scalar -> bool": (5.0 * n, lambda: upa > UPA_MIN), "int32 -> float64 (astype)": (12.0 * n, lambda: upa.astype(np.float64)),
                   "bool & bool": (3.0 * n, lambda: mask & mask), "~bool": (2.0 * n, lambda: ~mask),
                   "where(bool, int32, scalar)": (9.0 * n, lambda: where(mask, upa, -9999)),
                   "int32 max()": (4.0 * n, lambda: upa.max()), "bool count_nonzero()": (1.0 * n, lambda: mask.count_nonzero()),
                   "float32 min()": (4.0 * n, lambda: elev_dev.min())}
        for p in range(args.reps + 1):
            for name, (_, fn) in kernels.items():
                r = ew.link(name, fn)
                if hasattr(r, "free"):
                    r.free()
        say("  elementwise kernels alone (wall time of the call, allocation of the result included)")
        for s in ew.lines({k: v[0] for k, v in kernels.items()}):
            say(s)
    if len(digest) == 2:
        same = digest["numpy"] == digest["resident"]
        say(f"  results: {digest['numpy'][0]} drain cells, max HAND {digest['numpy'][1]:.3f}; sampled HAND bytes of the two forms "
            f"{'agree' if same else 'DIFFER'}")
        if not same:
            raise SystemExit("the two forms disagree")
    say(f"  allocator: {_hip.alloc_stats()}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


def main():
    args = parse()
    if args.child:
        return measure(args)
    # the parent never touches the GPU: the measurement is a fresh child under its own time limit
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    rc = subprocess.call(cmd)
    if rc in (124, 137):
        print(f"probe_resident_chain: the measurement was ended at its time limit ({args.timeout} s)", file=sys.stderr)
    sys.exit(rc)


if __name__ == "__main__":
    main()
