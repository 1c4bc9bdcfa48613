"""Token readout: the step from logits to tokens (``DiffusionPrefill::generate``'s predict /
``sample_token`` pair, diffusion_prefill/src/lib.rs:117-174).  Per row of logits [M, V] the greedy
token (the reference's ``max_by`` fold, ties and NaNs included), stats = {m, Z} (the row maximum and
the softmax denominator, so that the greedy token's probability is 1 / Z) and, on request, the
probabilities -- tokens and stats from one read of the logits.  The rule is pinned in
include/dllm_quant.h (section 8h) and is bit-reproducible on the host.  ``sample_tokens`` is the
sampling strategy the reference leaves open (sections 8j and 8k): temperature, top-k, top-p, min-p and
one seeded draw per row, pinned and reproducible in the same way.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._lib import check
from .quantization import _ptr, _stream

_ws = {}   # (device index, stream) -> grow-only u8 workspace of token_readout


def _workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


def _rows(logits):
    """The layout handling of both entry points: logits as device rows [M, V] of f16 or f32 with a
    dense last dimension -> (logits, single, M, V, ld)."""
    single = logits.dim() == 1
    if single:
        logits = logits.reshape(1, -1)
    if logits.dim() != 2:
        raise _lib.ShapeMismatch("logits must be [M, V]")
    if not logits.is_cuda or logits.dtype not in (torch.float16, torch.float32):
        logits = logits.to(device="cuda", dtype=torch.float16 if logits.dtype == torch.float16 else torch.float32)
    M, V = int(logits.shape[0]), int(logits.shape[1])
    if V == 0:
        raise _lib.InvalidParams("V == 0: no token to read out of an empty vocabulary")
    if M and (logits.stride(1) != 1 or (M > 1 and logits.stride(0) < V)):
        logits = logits.contiguous()
    ld = int(logits.stride(0)) if M > 1 else V
    return logits, single, M, V, ld


def token_readout(logits: torch.Tensor, probs: bool = False):
    """dllm_token_readout on logits [M, V] (f16 or f32; a 1-D tensor is one row) -> (tokens int32 [M],
    stats f32 [M, 2] = {m, Z}), and with ``probs`` also the probabilities f32 [M, V].  Rows may be
    strided (a column slice of a wider matrix is read in place); only the last dimension must be
    dense.  A row holding a NaN gets stats {NaN, NaN}, a row of -inf {-inf, 0}; both keep their token
    and touch no other row."""
    logits, single, M, V, ld = _rows(logits)
    L = _lib.load()
    dev = logits.device
    tokens = torch.empty(M, dtype=torch.int32, device=dev)
    stats = torch.empty(M, 2, dtype=torch.float32, device=dev)
    p = torch.empty(M, V, dtype=torch.float32, device=dev) if probs else None
    wsb = L.dllm_token_readout_workspace(M, V)
    ws = _workspace(dev, wsb)
    check(L.dllm_token_readout(_ptr(logits), _lib.F16 if logits.dtype == torch.float16 else _lib.F32, M, V, ld,
                               _ptr(tokens), _ptr(stats), _ptr(p), _ptr(ws), wsb, _stream()))
    if single:
        tokens, stats, p = tokens[0], stats[0], (p[0] if probs else None)
    return (tokens, stats, p) if probs else (tokens, stats)


def sample_tokens(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, seed: int = 0, offset: int = 0,
                  u: torch.Tensor = None, top_p: float = 1.0, min_p: float = 0.0, return_tau: bool = False):
    """dllm_token_sample on logits [M, V] (layouts as ``token_readout``) -> (tokens int32 [M], stats f32
    [M, 3] = {m, Z, p_token}): one token per row drawn from softmax(logits / temperature) restricted to
    the ``top_k`` largest logits (0 = all; ties at the k-th place are all kept).  Row b draws with the
    three uniforms of counter ``offset + b`` of the seeded stream ``seed``, or with ``u[b]`` (f32
    [M, 3]) when ``u`` is given.  A row with a NaN or +inf, or of -inf, gets token -1 and NaN stats.

    ``top_p`` < 1 keeps the smallest set of the largest survivors of top-k whose mass reaches ``top_p``
    (the nucleus), ``min_p`` > 0 keeps what has at least ``min_p`` times the maximum's probability
    (section 8k; ties at either threshold are all kept).  With either on, or with ``return_tau``, the
    call is dllm_token_sample_ex; ``return_tau`` makes stats [M, 4] = {m, Z, p_token, tau}, tau being
    the row's combined threshold on logits / temperature (-inf when no mask is on)."""
    logits, single, M, V, ld = _rows(logits)
    if top_k < 0:
        raise _lib.InvalidParams("top_k must not be negative")
    L = _lib.load()
    dev = logits.device
    if u is not None:
        u = u.to(device=dev, dtype=torch.float32).reshape(M, 3).contiguous()
    tokens = torch.empty(M, dtype=torch.int32, device=dev)
    dtype = _lib.F16 if logits.dtype == torch.float16 else _lib.F32
    if float(top_p) == 1.0 and float(min_p) == 0.0 and not return_tau:
        stats = torch.empty(M, 3, dtype=torch.float32, device=dev)
        wsb = L.dllm_token_sample_workspace(M, V, top_k)
        ws = _workspace(dev, wsb)
        check(L.dllm_token_sample(_ptr(logits), dtype, M, V, ld, float(temperature), int(top_k), _ptr(u),
                                  seed & (2 ** 64 - 1), offset & (2 ** 64 - 1), _ptr(tokens), _ptr(stats), _ptr(ws),
                                  wsb, _stream()))
    else:
        stats = torch.empty(M, 4, dtype=torch.float32, device=dev)
        wsb = L.dllm_token_sample_ex_workspace(M, V, top_k, float(top_p), float(min_p))
        ws = _workspace(dev, wsb)
        check(L.dllm_token_sample_ex(_ptr(logits), dtype, M, V, ld, float(temperature), int(top_k), float(top_p),
                                     float(min_p), _ptr(u), seed & (2 ** 64 - 1), offset & (2 ** 64 - 1), _ptr(tokens),
                                     _ptr(stats), _ptr(ws), wsb, _stream()))
        if not return_tau:
            stats = stats[:, :3]
    return (tokens[0], stats[0]) if single else (tokens, stats)


class TokenHead:
    """The vocabulary head: a ``QuantLinear`` with N = vocab (``DiffusionConfig.vocab_size``) followed
    by the readout.  ``out_dtype`` is the dtype of the logits the layer writes (f16 halves the bytes
    the readout reads; the readout widens them exactly)."""

    def __init__(self, linear, out_dtype=torch.float16):
        if out_dtype not in (torch.float16, torch.float32):
            raise _lib.UnsupportedOperation("out_dtype must be torch.float16 or torch.float32")
        self.linear, self.out_dtype = linear, out_dtype
        self.vocab_size = int(linear.N)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return self.linear.forward(x, out_dtype=self.out_dtype)

    def greedy(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [M, K] -> (tokens int32 [M], p_token f32 [M]): the greedy token of every row and its
        probability RN(1 / Z) (NaN for a row whose logits hold a NaN or +inf; inf for a row of -inf,
        whose Z is 0: such a row has no distribution)."""
        tokens, stats = token_readout(self.logits(x))
        return tokens, 1.0 / stats[:, 1]

    def sample(self, x: torch.Tensor, temperature: float = 1.0, top_k: int = 0, seed: int = 0,
               offset: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [M, K] -> (tokens int32 [M], p_token f32 [M]): ``sample_tokens`` of the layer's logits."""
        tokens, stats = sample_tokens(self.logits(x), temperature, top_k, seed, offset, top_p=top_p, min_p=min_p)
        return tokens, stats[:, 2]

    def probabilities(self, x: torch.Tensor) -> torch.Tensor:
        """x [M, K] -> softmax over the vocabulary, f32 [M, V]."""
        return token_readout(self.logits(x), probs=True)[2]
