"""A device entry point and its _host twin (csrc/host_rules.cpp) reject the same arguments with the same
status code and the same dllm_last_error() text: both call the one check function of the rule's header
(csrc/search_rule.hpp, neighbor_rule.hpp, token_args.hpp, dedup_rule.hpp).  Every device entry point
below makes these checks before its first HIP call, so all of them are in the table and nothing here
needs a GPU; no pointer is dereferenced, every call returns at a check."""
import ctypes as C

import pytest

P8 = C.c_void_p(4096)        # aligned for everything, never dereferenced
ODD = C.c_void_p(4100)       # 4-byte aligned only
BIG = 2 ** 40                # a workspace size no check finds too small
NAN, INF = float("nan"), float("inf")


def token(dev, host, extra):
    """Token entry points: (device call, host call) on M = 1, V = ld = 8, f32, T = 1, no mask; `extra`
    names what follows ld: nothing, the temperature, or the temperature and the two masks."""
    base = dict(logits=P8, dtype=0, M=1, V=8, ld=8, T=1.0, top_p=1.0, min_p=0.0)

    def args(a):
        a = {**base, **a}
        mid = {"": [], "T": [a["T"], 0, None, 0, 0], "Tpm": [a["T"], 0, a["top_p"], a["min_p"], None, 0, 0]}[extra]
        return a, [a["logits"], a["dtype"], a["M"], a["V"], a["ld"]] + mid

    def d(L, **kw):
        a, head = args(kw)
        tail = [P8, P8] + ([None] if extra == "" else []) + [P8, BIG, None]    # tokens, stats, (probs,) workspace
        return getattr(L, dev)(*head, *tail)

    def h(L, **kw):
        a, head = args(kw)
        return getattr(L, host)(*head, P8, P8, *([None] if extra == "" else []))

    return d, h


def pair(dev, host, order_dev, order_host, **base):
    """(device call, host call) from the argument order of each and the shared defaults."""
    def make(name, order):
        def call(L, **kw):
            a = {**base, "ws": P8, "wsb": BIG, "stream": None, **kw}
            return getattr(L, name)(*[a[k] for k in order])
        return call
    return make(dev, order_dev), make(host, order_host)


LOGITS = [dict(V=0, ld=0), dict(ld=7), dict(V=2 ** 31, ld=2 ** 31), dict(dtype=3), dict(dtype=-1),
          dict(V=0, ld=0, dtype=3), dict(V=2 ** 31, ld=2 ** 31 - 1), dict(V=2 ** 31, ld=2 ** 31, dtype=3),
          dict(dtype=3, M=0)]
TEMPS = [dict(T=t) for t in (0.0, -1.0, NAN, INF, 1e-45, 1e-39)] + [dict(dtype=3, T=0.0, M=0), dict(T=0.0, M=0),
                                                                      dict(V=0, ld=0, T=0.0)]
MASKS = [dict(top_p=v) for v in (0.0, -0.5, 1.5, NAN)] + [dict(min_p=v) for v in (-0.1, 1.5, NAN)] + [
    dict(T=0.0, top_p=0.0), dict(top_p=0.0, min_p=2.0), dict(top_p=0.0, M=0), dict(min_p=2.0, M=0)]
STORE = [dict(dim=0), dict(dim=65536), dict(rows=2 ** 31), dict(dim=0, rows=2 ** 31)]
KS = [dict(k=0), dict(k=257), dict(k=0, dim=0), dict(k=0, rows=2 ** 31), dict(k=0, nq=0), dict(dim=0, nq=0)]

SEARCH_T = ("codes", "rows", "dim", "scales", "zps", "table")
SEARCH_V = ("Q", "nq", "codes", "table", "rows", "dim", "k", "idx", "scores")
NEIGH_R = ("qcodes", "qtable", "nq", "codes", "table", "rows", "dim", "k", "threshold", "self_base", "idx", "scores")
DEDUP_R = ("hashes", "rows", "base", "table", "slots", "keep", "first", "kept_rows", "n_kept")
GATHER = ("codes", "dim", "ld", "kept_rows", "n_kept", "out", "out_ld")
W = ("ws", "wsb", "stream")
store = dict(codes=P8, rows=2, dim=4, scales=P8, zps=P8, table=P8)

TABLE = {
    "token_readout": (token("dllm_token_readout", "dllm_token_readout_host", ""), LOGITS),
    "token_sample": (token("dllm_token_sample", "dllm_token_sample_host", "T"), LOGITS + TEMPS),
    "token_sample_ex": (token("dllm_token_sample_ex", "dllm_token_sample_ex_host", "Tpm"), LOGITS + TEMPS + MASKS),
    "search_table": (pair("dllm_search_table", "dllm_search_table_host", SEARCH_T + ("stream",), SEARCH_T, **store), STORE),
    "search_vectors": (pair("dllm_search_vectors", "dllm_search_vectors_host", SEARCH_V + W, SEARCH_V,
                            Q=P8, nq=1, k=1, idx=P8, scores=P8, **store), STORE + KS),
    "neighbor_table": (pair("dllm_neighbor_table", "dllm_neighbor_table_host", SEARCH_T + ("stream",), SEARCH_T, **store),
                       STORE + [dict(table=ODD)]),
    "neighbor_rows": (pair("dllm_neighbor_rows", "dllm_neighbor_rows_host", NEIGH_R + W, NEIGH_R, qcodes=P8, qtable=P8,
                           nq=1, k=1, threshold=0.0, self_base=-1, idx=P8, scores=P8, **store),
                      STORE + KS + [dict(threshold=NAN), dict(self_base=-2), dict(self_base=2), dict(self_base=3),
                                    dict(self_base=0, nq=3), dict(k=0, threshold=NAN), dict(threshold=NAN, self_base=-2),
                                    dict(threshold=NAN, nq=0), dict(self_base=-2, nq=0), dict(qcodes=None),
                                    dict(qtable=None), dict(idx=None), dict(scores=None), dict(codes=None),
                                    dict(table=None), dict(qtable=ODD), dict(table=ODD), dict(qcodes=None, table=ODD)]),
    "hash_rows": (pair("dllm_hash_rows", "dllm_hash_rows_host", ("codes", "rows", "dim", "ld", "hashes", "stream"),
                       ("codes", "rows", "dim", "ld", "hashes"), codes=P8, rows=2, dim=4, ld=4, hashes=P8),
                  [dict(dim=0), dict(dim=65536, ld=65536), dict(ld=3), dict(rows=2 ** 31), dict(dim=0, rows=2 ** 31),
                   dict(ld=3, rows=2 ** 31), dict(dim=0, rows=0)]),
    "dedup_table_init": (pair("dllm_dedup_table_init", "dllm_dedup_table_init_host", ("table", "slots", "stream"),
                              ("table", "slots"), table=P8, slots=8),
                         [dict(slots=0), dict(slots=3), dict(slots=2 ** 57), dict(slots=3, table=None)]),
    "dedup_rows": (pair("dllm_dedup_rows", "dllm_dedup_rows_host", DEDUP_R + W, DEDUP_R, hashes=P8, rows=2, base=0,
                        table=P8, slots=8, keep=P8, first=P8, kept_rows=P8, n_kept=P8),
                   [dict(rows=2 ** 31), dict(base=2 ** 62), dict(slots=0), dict(slots=3), dict(slots=2 ** 57),
                    dict(table=ODD), dict(slots=2), dict(base=3), dict(rows=2 ** 31, base=2 ** 62),
                    dict(base=2 ** 62, slots=3), dict(slots=3, table=ODD), dict(table=ODD, slots=2),
                    dict(base=2 ** 62, rows=0), dict(slots=3, rows=0), dict(table=None, base=2 ** 62)]),
    "gather_rows": (pair("dllm_gather_rows", "dllm_gather_rows_host", GATHER + ("stream",), GATHER, codes=P8, dim=4, ld=4,
                         kept_rows=P8, n_kept=P8, out=P8, out_ld=4),
                    [dict(dim=0), dict(dim=65536, ld=65536, out_ld=65536), dict(ld=3), dict(out_ld=3),
                     dict(ld=3, out_ld=3), dict(dim=0, out_ld=0), dict(out_ld=3, codes=None)]),
}


@pytest.mark.parametrize("rule", sorted(TABLE))
def test_device_and_host_reject_alike(dllm, rule):
    L = dllm._lib.load()
    (dev, host), cases = TABLE[rule]
    for bad in cases:
        got = []
        for call in (dev, host):
            rc = call(L, **bad)
            got.append((rc, L.dllm_last_error()))
        assert got[0] == got[1], (rule, bad, got)
        assert got[0][0] != 0 and got[0][1], (rule, bad, got)      # a rejection, with a message


def test_v0_wordings_stay_apart(dllm):
    """The readout and the sampling entry points word an empty vocabulary differently (8h, 8j)."""
    L = dllm._lib.load()
    texts = []
    for rule in ("token_readout", "token_sample", "token_sample_ex"):
        (dev, host), _ = TABLE[rule]
        assert dev(L, V=0, ld=0) == host(L, V=0, ld=0) == dllm._lib.ERR_INVALID_PARAMS
        texts.append(L.dllm_last_error())
    assert b"read out of" in texts[0] and b"sample from" in texts[1] and texts[1] == texts[2]
