"""ctypes binding of libyt8m_hip.so, computed from include/yt8m_hip.h: the header is the contract, and the argument types, the struct
mirrors and the constants below are what it declares.  Fails loudly when the library is missing (the product has no CPU /
eager-PyTorch fallback for any hot op) and when the header holds anything the parser does not recognise (it never guesses a type)."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YT8M_LIB", os.path.join(_HERE, "libyt8m_hip.so"))  # YT8M_LIB: A/B builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "yt8m_hip.h")

P = ctypes.c_void_p                # every pointer whose C type says no more: device memory, streams, handles, host out-parameters
PP = ctypes.POINTER(P)             # pointer to pointers (arrays of device pointers, yt8m_stream_t*, void**)
STREAM_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)       # yt8m_stream_hook (bound as P: callers pass its address)
STRUCT_NAMES = {"yt8m_gemm_problem": "GemmProblem", "yt8m_persist_bwd_images": "PersistBwdImages", "yt8m_lstm_stack_desc": "LstmStackDesc",
                "yt8m_wimg_demand": "WimgDemand", "yt8m_wimg_spec": "WimgSpec", "yt8m_wimg_job": "WimgJob", "yt8m_opt_ranges": "OptRanges"}
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
            "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = ("void", "char", "uint8_t")       # types the header only ever points at


class Yt8mHipError(RuntimeError):
    pass


def _refuse(what, text):
    raise Yt8mHipError("include/yt8m_hip.h: unrecognised %s: %r" % (what, " ".join(text.split())))


def _int(text, what, context):
    try:
        return int(text, 0)
    except ValueError:
        _refuse(what, context)


_STATEMENT = re.compile(r"\s*(?:typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<members>[^{}]*)\}\s*(?P=struct)\s*;|enum\s+\w+\s*\{(?P<enum>[^{}]*)\}\s*;"
                        r"|typedef\s+[^;{}()]+\(\s*\*\s*(?P<hook>\w+)\s*\)\s*\([^;{}()]*\)\s*;|typedef\s+(?P<typedef>[^;{}()]+);"
                        r"|(?P<ret>[^;{}()]+?)\b(?P<function>\w+)\s*\((?P<params>[^;{}()]*)\)\s*;)")
_SPECIFIER = re.compile(r"\s*((?:const\s+)?(?:enum\s+)?\w+)\s*(.*)", re.S)
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\s*)?)*)(\w*)\s*(?:\[(\d+)\])?\s*")


def _declare(text, types, role, of):
    """[(name, ctype)] of one C declaration `specifier declarator, ...` in the role "parameter", "member", "typedef" or "return type"
    of the function, struct or typedef `of` (for the error text)."""
    what = "%s of %s" % (role, of)
    m = _SPECIFIER.fullmatch(text)
    if not m:
        _refuse(what, text)
    spec = " ".join(m[1].split())
    base = spec[6:] if spec.startswith("const ") else spec
    t = ctypes.c_int if base.startswith("enum ") else types.get(base)
    out = []
    for declarator in m[2].split(","):
        d = _DECLARATOR.fullmatch(declarator)
        if not d or bool(d[2]) == (role == "return type") or (d[3] and role != "member"):
            _refuse(what, text)
        depth = d[1].count("*") + (t is P)        # a typedef of a pointer (yt8m_stream_t, yt8m_stream_hook) is one level itself
        if t is None and not (depth and base in _POINTEES) and (spec, role, depth) != ("void", "return type", 0):
            _refuse("type %r in %s" % (spec, what), text)
        if depth > 2:
            _refuse(what, text)
        is_struct = isinstance(t, type) and issubclass(t, ctypes.Structure)
        if depth == 2:
            ct = ctypes.POINTER(ctypes.c_char_p) if spec == "const char" else PP
        elif depth == 1:
            ct = ctypes.c_char_p if (spec, role) == ("const char", "return type") else \
                ctypes.POINTER(t) if is_struct and role != "member" else P
        else:
            ct = t
        out.append((d[2], ct * int(d[3]) if d[3] else ct))
    return out


def parse_header(text, struct_names=STRUCT_NAMES):
    """(signatures, structs, constants) of a C header in the dialect of include/yt8m_hip.h.  signatures: function name -> (restype,
    [argtypes]); structs: C struct name -> ctypes.Structure mirror; constants: enumerators and integer #defines.  Raises Yt8mHipError,
    naming the text, for anything it does not recognise."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, structs, constants, types, body, cplusplus = {}, {}, {}, dict(_SCALARS), [], False
    for line in text.splitlines():
        m = re.match(r"\s*#\s*(\w+)\s*(.*)", line)
        if not m:
            body.append("" if cplusplus else line)
            continue
        cplusplus = (m[1], m[2].strip()) == ("ifdef", "__cplusplus") or (cplusplus and m[1] != "endif")
        define = re.fullmatch(r"(\w+)\s+(\S.*?)\s*", m[2]) if m[1] == "define" else None
        if define:
            constants[define[1]] = _int(define[2], "#define", line)
    text, pos = "\n".join(body), 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            _refuse("declaration", text[pos:].strip().split(";")[0])
        pos = m.end()
        if m["struct"]:
            fields = [f for member in m["members"].split(";") if member.strip() for f in _declare(member, types, "member", m["struct"])]
            name = struct_names.get(m["struct"], m["struct"])
            types[m["struct"]] = structs[m["struct"]] = type(name, (ctypes.Structure,), {
                "_fields_": fields, "__doc__": "%s (include/yt8m_hip.h)." % m["struct"]})
        elif m["enum"] is not None:
            value = -1
            for e in m["enum"].split(","):
                name, _, given = (s.strip() for s in e.partition("="))
                if name or given:
                    if not re.fullmatch(r"\w+", name):
                        _refuse("enumerator", e)
                    constants[name] = value = _int(given, "enumerator", e) if given else value + 1
        elif m["hook"]:
            types[m["hook"]] = P
        elif m["typedef"]:
            (name, ct), = _declare(m["typedef"], types, "typedef", "a pointer or scalar")
            if ct is not P and ct not in _SCALARS.values():
                _refuse("typedef", m["typedef"])
            types[name] = ct
        else:
            params = m["params"].strip()
            args = [] if params in ("", "void") else [_declare(p, types, "parameter", m["function"])[0][1] for p in params.split(",")]
            signatures[m["function"]] = (_declare(m["ret"], types, "return type", m["function"])[0][1], args)
    return signatures, structs, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise Yt8mHipError("the C header the binding is computed from cannot be read: %s (%s)" % (HEADER_PATH, e))


# name -> (restype, argtypes) of every function, the mirror of every struct, every enumerator and integer #define of include/yt8m_hip.h
SIGNATURES, STRUCTS, CONSTANTS = parse_header(_read_header())
globals().update({py: STRUCTS[c] for c, py in STRUCT_NAMES.items()})     # GemmProblem, PersistBwdImages, LstmStackDesc, Wimg*, OptRanges
DESC = ctypes.POINTER(STRUCTS["yt8m_lstm_stack_desc"])
# The one struct pointer that is a DEVICE address, which its C type cannot say: the caller passes the address, not a mirror.
SIGNATURES["yt8m_adam_tiles"][1][4] = P                                  # const yt8m_wimg_job* jobs

# The ABI this host binds (include/yt8m_hip.h, yt8m_abi_version): workspace layouts and argument meanings, not just symbols.
ABI_VERSION = 4

_lib = None


def lib():
    """Returns the loaded CDLL; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Yt8mHipError(
                "libyt8m_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C youtube-8m_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # torch first: its bundled HIP runtime must be the one the process initialises.  Loaded the other way round (build() then smoke()
        # in one process on the GPU box) the library's launches fail with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.yt8m_abi_version() != ABI_VERSION:
            raise Yt8mHipError("libyt8m_hip.so speaks ABI %d, this host was written for ABI %d: rebuild with `make -C youtube-8m_amd/csrc`"
                               % (L.yt8m_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


_STATUS = {v: k for k, v in CONSTANTS.items() if k.startswith("YT8M_E_")}       # enum yt8m_status


def check(status):
    if status != 0:
        msg = lib().yt8m_last_error().decode("utf-8", "replace")
        exc = ValueError if status in (-1, -2) else Yt8mHipError
        raise exc("%s: %s" % (_STATUS.get(status, status), msg))
