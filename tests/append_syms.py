"""The append kernels of libqmha.so by symbol (qmha_prepass.hip): two templates per precision,
qmha_kv_append_{int8,f16}_kernel<D, Row> and qmha_kv_rows_{int8,f16}_kernel<D, Src, Dst>, read from `nm`'s host stubs.
The CPU tests of the cache family pin their own instances with `append` / `rows` and the whole family with `check_family`.
"""
import re

SIZES = {"int8": ["128", "32", "64"], "f16": ["128", "64"]}
ROWS = ("HostRow", "PlacedRow")
SRCS = ("UniformRows", "PackedRows")
DSTS = ("ContiguousRows", "PagedTable")


def append(syms, row=None):
    """Every (template, row policy, d) of the append template, as a sorted list; of one policy with `row`."""
    got = re.findall(r"__device_stub__(qmha_kv_append_(?:int8|f16)_kernel)ILi(\d+)ENS_\d+([A-Za-z]+)EEEv", syms)
    return sorted((t, r, d) for t, d, r in got if row in (None, r))


def rows(syms, src=None, dst=None):
    """Every (template, source policy, destination policy, d) of the rows template, as a sorted list."""
    got = re.findall(r"__device_stub__(qmha_kv_rows_(?:int8|f16)_kernel)ILi(\d+)ENS_\d+([A-Za-z]+)ENS_\d+([A-Za-z]+)EEEv", syms)
    return sorted((t, s, e, d) for t, d, s, e in got if src in (None, s) and dst in (None, e))


def want_append(row_policies=ROWS):
    return sorted((f"qmha_kv_append_{p}_kernel", r, d) for p, ds in SIZES.items() for d in ds for r in row_policies)


def want_rows(srcs=SRCS, dsts=DSTS):
    return sorted((f"qmha_kv_rows_{p}_kernel", s, e, d) for p, ds in SIZES.items() for d in ds for s in srcs for e in dsts)


def check_family(syms):
    """Exactly the ten append and the twenty rows instances: each (template, policies, d) once, no policy combination
    beyond the two and the four, and no stub of the family under any other name or argument list."""
    assert append(syms) == want_append(), append(syms)
    assert rows(syms) == want_rows(), rows(syms)
    stubs = re.findall(r"__device_stub__(qmha_kv_\w+)", syms)
    assert len(stubs) == len(set(stubs)) == 30, sorted(stubs)
    assert len([s for s in stubs if s.startswith("qmha_kv_append_")]) == 10
    assert len([s for s in stubs if s.startswith("qmha_kv_rows_")]) == 20
