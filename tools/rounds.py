"""What the kernel bench tools of this directory share: the yardstick (tools/yardstick.hip, the same bytes with no
arithmetic), HIP events on the launching stream, a quantizer module as a forward and a backward candidate, and the
protocol -- interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when
the timed launch starts), median / min over the rounds.  A candidate is a name and a call; 'fwd' / 'bwd' end the name."""
import ctypes
import functools
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'build', 'tools', 'libyardstick.so')


def ev():
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


@functools.lru_cache(None)
def _yardstick_lib(device):
    """libyardstick.so and its sink on `device`, loaded once"""
    import torch
    yl = ctypes.CDLL(SO)
    yl.yardstick.restype = ctypes.c_int
    yl.yardstick.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]
    return yl, torch.zeros(4, device=device, dtype=torch.int32)


def yardstick(x, g, o):
    """-> yard(mode, nt, ch, form, blocks): one launch of tools/yardstick.hip over the bytes of x (g: the second stream
    of a triad, o: the output), on the current stream"""
    import torch
    yl, sink = _yardstick_lib(x.device)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = x.numel() * x.element_size()

    def yard(mode, nt, ch, form, blocks):
        rc = yl.yardstick(mode, nt, ch, form, blocks, x.data_ptr(), g.data_ptr(), o.data_ptr(), sink.data_ptr(), nbytes,
                          stream)
        assert rc == 0, rc
    return yard


def yardstick_cands(yard, tag='(d)', persistent=True):
    """the ceiling candidates: read + write ('copy') and two reads + write ('triad'), a small sweep"""
    cands = {}
    for mode, mname in ((1, 'copy'), (2, 'triad')):
        for nt in (1, 0):
            for ch in (2, 4, 8):
                cands['%s %s unit nt=%d ch=%d' % (tag, mname, nt, ch)] = lambda m=mode, n=nt, c=ch: yard(m, n, c, 0, 0)
            if persistent:
                cands['%s %s persistent nt=%d ch=4 blocks=2048' % (tag, mname, nt)] = \
                    lambda m=mode, n=nt: yard(m, n, 4, 1, 2048)
    return cands


def module_pair(q, w, grad):
    """forward and backward of a quantizer module as two timed calls; the backward runs on the graph the last forward
    left"""
    state = {}

    def fwd():
        w.grad = None
        state['y'] = q(w)[0]

    def bwd():
        if 'y' not in state:
            fwd()
        state.pop('y').backward(grad)
    return fwd, bwd


def timed_rounds(cands, rounds, warmup=1):
    """-> {name: [ms per round]}.  A module's backward ('module' in its name, ending in 'bwd') consumes its graph: its
    warm call is forward + backward, then a fresh forward, then the timed call."""
    import torch
    names = list(cands)
    for _ in range(warmup):
        for name in names:   # (a module's backward needs its forward before it)
            cands[name]()
    torch.cuda.synchronize()
    res = {name: [] for name in names}
    for _ in range(rounds):
        pairs = []
        for name in names:
            fn = cands[name]
            fn()
            if 'module' in name and name.endswith('bwd'):
                cands[name[:-3] + 'fwd']()
            a = ev()
            out = fn()
            pairs.append((name, a, ev()))
            del out
        torch.cuda.synchronize()
        for name, a, b in pairs:
            res[name].append(a.elapsed_time(b))
    return res


def report(res, nbytes, width, ceiling='(d)'):
    """one line per candidate: median / min ms and the x-sized passes per median (2 forward, 3 backward or triad)
    -> (medians, the best median per kind of the `ceiling` candidates)"""
    med = {name: statistics.median(ts) for name, ts in res.items()}
    best = {}
    for name, ts in res.items():
        passes = 3 if ('bwd' in name or 'triad' in name) else 2
        print('%-*s %8.4f / %8.4f ms  %5.2f TB/s' % (width, name, med[name], min(ts), passes * nbytes / med[name] / 1e9))
        if name.startswith(ceiling):
            kind = name.split(' ')[1]
            best[kind] = min(best.get(kind, med[name]), med[name])
    return med, best
