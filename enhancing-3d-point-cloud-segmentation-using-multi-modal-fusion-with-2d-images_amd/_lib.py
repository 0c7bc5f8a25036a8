"""ctypes binding of libmvkpconv.so (C ABI: include/mvkpconv.h, with include/mvkpconv_scene.h,
include/mvkpconv_train.h, include/mvkpconv_sphere.h and include/mvkpconv_decoder.h beside it).

There is NO fallback: if the HIP library is missing or stale this module raises. PyTorch is used
only as the owner of device memory and streams -- every signature is plain pointers and sizes.

The header is the only declaration of the ABI. parse_header() reads it when this module is imported -- prototypes,
struct layouts and integer #defines -- and one mapping from C type to ctypes type turns that into restype / argtypes
and the Structure classes. The parser knows three forms (function declaration, struct typedef, #define of an integer)
and raises with the line number on everything else: a header it cannot read completely is an error, never a guess.
tests/test_abi_binding_cpu.py lets the host compiler check what it read.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmvkpconv.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "mvkpconv.h")
SCENE_HEADER_PATH = os.path.join(_HERE, "..", "include", "mvkpconv_scene.h")
TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "mvkpconv_train.h")
SPHERE_HEADER_PATH = os.path.join(_HERE, "..", "include", "mvkpconv_sphere.h")
DECODER_HEADER_PATH = os.path.join(_HERE, "..", "include", "mvkpconv_decoder.h")

# canonical C type -> ctypes type. A pointer that is not listed is POINTER(Structure) for a struct of the header and
# c_void_p otherwise (device and host arrays alike are passed as addresses).
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
          "const char*": C.c_char_p}
_SCALARS = frozenset(t for t in CTYPES if not t.endswith("*"))
_POINTEES = _SCALARS | {"void", "char", "uint8_t", "uint16_t"}      # what a pointer may point to, besides a struct
_INTEGER = r"-?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)"
_DIRECTIVE = re.compile(r"\s*#\s*(?:include\s*<[\w./]+>|ifdef\s+__cplusplus|ifndef\s+\w+_H|endif"      # guard, not a switch
                        r"|define\s+(\w+)(?:\s+(%s))?)\s*" % _INTEGER)
_STRUCT = re.compile(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(mvk_\w+)\s*;")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(mvk_\w+)\s*\(([^(){};]*)\)\s*;")


def parse_header(text):
    """(FUNCTIONS, STRUCTS, CONSTANTS) of a header in the style of include/mvkpconv.h:
    FUNCTIONS {name: (return type, ((type, parameter name), ...))}, STRUCTS {name: ((type, field name), ...)}, both in
    header order with types in canonical spelling ('const float*', 'int64_t'), CONSTANTS {MVK_NAME: int}."""
    functions, structs, constants = {}, {}, {}

    def fail(pos, what):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        raise ValueError("mvkpconv.h line %d: %s" % (text.count("\n", 0, pos) + 1, what))

    def canonical(pos, spelling):
        """[const] <known type word> [*], or it raises."""
        tokens = re.findall(r"\w+|\S", spelling)
        const = tokens[:1] == ["const"]
        base, stars = "".join(tokens[const:const + 1]), tokens[const + 1:]
        if not (stars == [] and not const and base in _SCALARS
                or stars == ["*"] and (base in _POINTEES or base in structs)):
            fail(pos, "unsupported type %r" % " ".join(tokens))
        return "const " * const + base + "*" * len(stars)

    def declarator(pos, spelling):
        """'const float* x' -> ('const float*', 'x')"""
        m = re.fullmatch(r"(.*[\s*])([A-Za-z_]\w*)\s*", spelling, re.S)
        if not m or m.group(2) == "const" or m.group(2) in _POINTEES:
            fail(pos, "expected '<type> <name>', found %r" % spelling.strip())
        return canonical(pos, m.group(1)), m.group(2)

    # a comment becomes a blank and its line breaks, a preprocessor line an empty line: line numbers stay the header's
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    lines = text.split("\n")
    for i, line in enumerate(lines):
        if line.lstrip().startswith("#"):
            m = _DIRECTIVE.fullmatch(line)
            name, value = m.groups() if m else (None, None)
            if not m or (name is not None and (name.startswith("MVK_") != (value is not None) or name in constants)):
                raise ValueError("mvkpconv.h line %d: unsupported preprocessor line %r" % (i + 1, line.strip()))
            if value is not None:
                constants[name] = int(value, 0)
            lines[i] = ""
    text = "\n".join(lines)

    block = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    if not block:
        fail(0, 'expected one extern "C" { ... } block around all declarations')
    pos, end = block.start(1), block.end(1)
    while True:
        pos = re.compile(r"\s*").match(text, pos, end).end()
        if pos == end:
            return functions, structs, constants
        s = _STRUCT.match(text, pos, end)
        f = None if s else _FUNCTION.match(text, pos, end)
        if (s or f) and (s or f).group(2) in functions.keys() | structs.keys():
            fail(pos, "%s is declared twice" % (s or f).group(2))
        if s:
            fields, at = [], s.start(1)
            *statements, tail = s.group(1).split(";")
            if tail.strip() or not statements:
                fail(s.end(1) - len(tail), "struct %s: expected 'type name;' fields" % s.group(2))
            for statement in statements:      # 'float eps, momentum, slope' declares three fields
                first, *more = statement.split(",")
                ctype, name = declarator(at, first)
                if more and (ctype.endswith("*") or not all(re.fullmatch(r"\s*[A-Za-z_]\w*\s*", n) for n in more)):
                    fail(at, "only scalar fields share a declaration, found %r" % statement.strip())
                fields += [(ctype, n.strip()) for n in [name] + more]
                at += len(statement) + 1
            structs[s.group(2)] = tuple(fields)
        elif f:
            params, at = [], f.start(3)
            for spelling in f.group(3).split(",") if f.group(3).strip() != "void" else ():
                params.append(declarator(at, spelling))
                at += len(spelling) + 1
            functions[f.group(2)] = (canonical(pos, f.group(1)), tuple(params))
        else:
            fail(pos, "neither a function declaration nor a struct typedef: %r" % text[pos:end].split("\n")[0].strip())
        pos = (s or f).end()


def _bind(functions, structs):
    """({struct name: Structure class}, {function name: (restype, argtypes)}) through CTYPES."""
    classes = {}

    def ctype(t):
        if t in CTYPES:
            return CTYPES[t]
        assert t.endswith("*"), t
        pointee = t[6 * t.startswith("const "):-1]
        return C.POINTER(classes[pointee]) if pointee in classes else C.c_void_p

    for name, fields in structs.items():
        classes[name] = type("".join(w.capitalize() for w in name.split("_")[1:]), (C.Structure,),
                             {"_fields_": [(n, ctype(t)) for t, n in fields], "__doc__": name + " (include/mvkpconv.h)"})
    return classes, {name: (ctype(ret), [ctype(t) for t, _ in params]) for name, (ret, params) in functions.items()}


def _read_header(path=None, name="mvkpconv.h"):
    path = HEADER_PATH if path is None else path
    if not os.path.exists(path):
        raise RuntimeError(
            "include/%s is not there (%s). The binding reads every prototype of libmvkpconv.so from it -- "
            "run the package from a checkout of the repository; there is no second copy of the C ABI." % (name, path))
    with open(path) as f:
        return f.read()


FUNCTIONS, STRUCTS, CONSTANTS = parse_header(_read_header())
_CLASSES, _PROTOTYPES = _bind(FUNCTIONS, STRUCTS)
EXPORTS = tuple(FUNCTIONS)
ABI_VERSION = CONSTANTS["MVK_ABI_VERSION"]

# the second header (whole-scene inputs, csrc/scene_inputs.hip): same parser, same library, its own tables -- the
# declaration of ABI 9 above is not extended by it. It declares functions and constants only.
SCENE_FUNCTIONS, _scene_structs, SCENE_CONSTANTS = parse_header(_read_header(SCENE_HEADER_PATH, "mvkpconv_scene.h"))
if _scene_structs or SCENE_FUNCTIONS.keys() & FUNCTIONS.keys() or SCENE_CONSTANTS.keys() & CONSTANTS.keys():
    raise ValueError("mvkpconv_scene.h: it may declare neither a struct nor a name of mvkpconv.h")
_SCENE_PROTOTYPES = _bind(SCENE_FUNCTIONS, {})[1]

# the third header (training batches from resident scenes, csrc/train_inputs.hip): the same again
TRAIN_FUNCTIONS, _train_structs, TRAIN_CONSTANTS = parse_header(_read_header(TRAIN_HEADER_PATH, "mvkpconv_train.h"))
if (_train_structs or TRAIN_FUNCTIONS.keys() & (FUNCTIONS.keys() | SCENE_FUNCTIONS.keys())
        or TRAIN_CONSTANTS.keys() & (CONSTANTS.keys() | SCENE_CONSTANTS.keys())):
    raise ValueError("mvkpconv_train.h: it may declare neither a struct nor a name of the other two headers")
_TRAIN_PROTOTYPES = _bind(TRAIN_FUNCTIONS, {})[1]

# the fourth header (sphere batches of the KPFCNN networks, csrc/sphere_inputs.hip): the same again
SPHERE_FUNCTIONS, _sphere_structs, SPHERE_CONSTANTS = parse_header(_read_header(SPHERE_HEADER_PATH, "mvkpconv_sphere.h"))
if (_sphere_structs
        or SPHERE_FUNCTIONS.keys() & (FUNCTIONS.keys() | SCENE_FUNCTIONS.keys() | TRAIN_FUNCTIONS.keys())
        or SPHERE_CONSTANTS.keys() & (CONSTANTS.keys() | SCENE_CONSTANTS.keys() | TRAIN_CONSTANTS.keys())):
    raise ValueError("mvkpconv_sphere.h: it may declare neither a struct nor a name of the other three headers")
_SPHERE_PROTOTYPES = _bind(SPHERE_FUNCTIONS, {})[1]

# the fifth header (the decoder's unary layers as two products, csrc/gemm.hip): the same again, functions only
DECODER_FUNCTIONS, _decoder_structs, _decoder_constants = parse_header(_read_header(DECODER_HEADER_PATH, "mvkpconv_decoder.h"))
if (_decoder_structs or _decoder_constants
        or DECODER_FUNCTIONS.keys() & (FUNCTIONS.keys() | SCENE_FUNCTIONS.keys() | TRAIN_FUNCTIONS.keys() | SPHERE_FUNCTIONS.keys())):
    raise ValueError("mvkpconv_decoder.h: it may declare neither a struct, a constant nor a name of the other four headers")
_DECODER_PROTOTYPES = _bind(DECODER_FUNCTIONS, {})[1]
BnFwdProblem, BnBwdProblem = _CLASSES["mvk_bn_fwd_problem"], _CLASSES["mvk_bn_bwd_problem"]
BnFinish, ATransform = _CLASSES["mvk_bn_finish"], _CLASSES["mvk_a_transform"]
RevList, RegLayer = _CLASSES["mvk_rev_list"], _CLASSES["mvk_reg_layer"]

_lib = None
_owner_pid = None

FORK_MESSAGE = ("the MV-KPConv HIP library was initialised in process %d and is being called from its forked child %d: "
                "a HIP context does not survive fork(). Start DataLoader workers with multiprocessing_context='spawn', "
                "or let the workers emit only stacked points / lengths and build the pyramid "
                "(datasets.common.segmentation_inputs_sphere) in the main process -- see INTEGRATION.md")


def _check_process():
    """Loud failure instead of a hang when a forked worker (the reference builds the pyramid in
    num_workers forked DataLoader processes, train_ScanNet_sphere.py:365-377) calls into the library."""
    pid = os.getpid()
    if _owner_pid is not None and pid != _owner_pid:
        raise RuntimeError(FORK_MESSAGE % (_owner_pid, pid))
    try:
        import torch
        if torch.cuda._is_in_bad_fork():
            raise RuntimeError(FORK_MESSAGE % (os.getppid(), pid))
    except (ImportError, AttributeError):
        pass


def lib():
    """The loaded library. Raises (never falls back) when it is absent or has the wrong ABI, or when the
    caller is a forked child of the process that initialised it."""
    global _lib, _owner_pid
    _check_process()
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmvkpconv.so is not built (%s). Run `python __graft_entry__.py build` -- there is "
                "no CPU fallback for the MV-KPConv hot path." % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_PROTOTYPES.items()) + list(_SCENE_PROTOTYPES.items()) + list(_TRAIN_PROTOTYPES.items()) \
                + list(_SPHERE_PROTOTYPES.items()) + list(_DECODER_PROTOTYPES.items()):
            fn = getattr(l, name)          # AttributeError = missing export = stale build: loud
            fn.restype = res
            fn.argtypes = args
        if l.mvk_abi_version() != ABI_VERSION:
            raise RuntimeError("libmvkpconv.so ABI %d != expected %d; rebuild" % (l.mvk_abi_version(), ABI_VERSION))
        _lib = l
        _owner_pid = os.getpid()
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().mvk_last_error().decode("utf-8", "replace"))
