"""What every per-feature host test asks of its entry points at the C boundary, in one place."""
import os
import re

import yt8m_amd._lib as L
from conftest import ROOT


def declared_bound_exported(symbols, returns="int"):
    """Each symbol is declared in include/yt8m_hip.h with a return type that matches the regex `returns`, bound in _lib.SIGNATURES and
    exported by the built library.  Returns (header text, loaded library) for the checks that are the feature's own."""
    src = open(os.path.join(ROOT, "include", "yt8m_hip.h")).read()
    lib = L.lib()
    for name in symbols:
        assert re.search(r"\b%s\s+%s\s*\(" % (returns, name), src), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    return src, lib
