"""Read sets of the timing tools (time_anchors.py, time_smems.py): 101-bp windows of a text on the device, planted
substitutions, and a warmed device-event timer.  Reads no arguments and touches no device on import."""
import torch

L = 101


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def plant(q, m, seed):
    """m substitutions at distinct random positions of every row of q (uint8[n, L] on the device); letters outside ACGT become A"""
    if m == 0:
        return q
    gen = torch.Generator(device=q.device)
    gen.manual_seed(seed)
    q = q.clone()
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=q.device)
    code = torch.full((256,), 3, dtype=torch.int64, device=q.device)
    code[lut.long()] = torch.arange(4, device=q.device)
    rows = torch.arange(q.shape[0], device=q.device)
    cols = torch.argsort(torch.rand(q.shape, device=q.device, generator=gen), dim=1)[:, :m]
    for j in range(m):
        c = cols[:, j]
        old = code[q[rows, c].long()]
        q[rows, c] = lut[(old + torch.randint(1, 4, (q.shape[0],), device=q.device, generator=gen)) % 4]
    return q


def windows(text_d, count, seed):
    """windows of the text at uniform positions, whatever they hold"""
    gen = torch.Generator(device=text_d.device)
    gen.manual_seed(seed)
    pos = torch.randint(0, text_d.numel() - 1 - L, (count,), device=text_d.device, generator=gen)
    return text_d[pos[:, None] + torch.arange(L, device=text_d.device)[None, :]]
