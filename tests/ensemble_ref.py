"""The geometric self-ensemble restated for the tests, in plain torch ops on any device: the eight members, their inverses and
the fp32 accumulation in member order (HATEngine.forward_ensemble's definition).  Shares no code with the product
or with tests/golden/gen_golden_ensemble.py."""
import torch


def member(x: torch.Tensor, i: int) -> torch.Tensor:
    """T_i x on the last two axes (H, W): bit 0 of i reverses W, then bit 1 reverses H, then bit 2 swaps H and W."""
    v, h, t = i & 1, (i >> 1) & 1, (i >> 2) & 1
    x = torch.flip(x, dims=[-1]) if v else x
    x = torch.flip(x, dims=[-2]) if h else x
    x = torch.transpose(x, -2, -1) if t else x
    return x.contiguous()


def undo(y: torch.Tensor, i: int) -> torch.Tensor:
    """T_i^-1 y: the swap is undone first, then the H reversal, then the W reversal."""
    v, h, t = i & 1, (i >> 1) & 1, (i >> 2) & 1
    y = torch.transpose(y, -2, -1) if t else y
    y = torch.flip(y, dims=[-2]) if h else y
    y = torch.flip(y, dims=[-1]) if v else y
    return y.contiguous()


def member_outputs(net, x: torch.Tensor, n: int):
    """[T_i^-1 net(T_i x) for i < n]"""
    return [undo(net(member(x, i)), i) for i in range(n)]


def accumulate(outs, n: int) -> torch.Tensor:
    """acc = 0; acc = acc + (1 / n) * outs[i] for i = 0 .. n-1, in fp32"""
    acc = torch.zeros_like(outs[0], dtype=torch.float32)
    for i in range(n):
        acc = acc + (1.0 / n) * outs[i].to(torch.float32)
    return acc


def ensemble(net, x: torch.Tensor, n: int) -> torch.Tensor:
    return accumulate(member_outputs(net, x, n), n)
