"""The C ABI as the headers declare it: include/pn2hip.h and include/pn2plan.h parsed into
ctypes signatures, `PN2_*` constants and `ctypes.Structure` classes (_lib.py binds them).

The headers are the single source: nothing here names a function, a constant or a field. What
the parser does not understand raises HeaderError with the header and the declaration; it
never guesses a type. Pure Python: imports neither torch nor the library.
"""
import ast
import ctypes
import os
import re

HEADERS = ("pn2hip.h", "pn2plan.h")

_SCALARS = {
    "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
    "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32,
    "uint64_t": ctypes.c_uint64,
}
_POINTER = ctypes.c_void_p  # callers pass ints, None and ctypes arrays
_STRUCT = re.compile(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(PN2_\w+)(?:[ \t]+(.*?))?[ \t]*$", re.M)


class HeaderError(Exception):
    """A declaration the parser does not understand."""


def _int_expr(node):
    """Integers, unary minus, shifts, + and * (parentheses come with the tree)."""
    if isinstance(node, ast.Constant) and type(node.value) is int:
        return node.value
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
        return -_int_expr(node.operand)
    if isinstance(node, ast.BinOp):
        a, b = _int_expr(node.left), _int_expr(node.right)
        if isinstance(node.op, ast.LShift):
            return a << b
        if isinstance(node.op, ast.RShift):
            return a >> b
        if isinstance(node.op, ast.Add):
            return a + b
        if isinstance(node.op, ast.Mult):
            return a * b
    raise ValueError(ast.dump(node))


def _constant(text):
    text = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b", r"\1", text)  # 1LL, 64u
    return _int_expr(ast.parse(text.strip(), mode="eval").body)


class Abi:
    """functions: name -> (restype, argtypes); constants: PN2_NAME -> int; structs: typedef
    name -> ctypes.Structure subclass. read() adds one header's declarations; typedefs carry
    over to the headers read after it (pn2plan.h uses pn2hip.h's pn2_stream_t)."""

    def __init__(self):
        self.functions, self.constants, self.structs = {}, {}, {}
        self._types = dict(_SCALARS)
        self._opaque = {"void", "char"}  # what a returned pointer may point to

    def _scalar(self, ctype, where):
        ctype = " ".join(t for t in ctype.split() if t != "const")
        if ctype not in self._types:
            raise HeaderError(f"{where}: unknown type '{ctype}'")
        return self._types[ctype]

    def _param(self, decl, where):
        if "*" in decl or "[" in decl:
            return _POINTER
        tokens = decl.split()
        name = tokens.pop() if len(tokens) > 1 else "<unnamed>"
        return self._scalar(" ".join(tokens), f"{where}, parameter '{name}'")

    def _function(self, ret, name, params, where):
        ret = ret.strip()
        if "*" in ret:
            base = " ".join(t for t in ret.replace("*", " ").split() if t != "const")
            if base not in self._opaque:
                raise HeaderError(f"{where}: unknown return type '{ret}'")
            res = ctypes.c_char_p if base == "char" else _POINTER
        else:
            res = None if ret == "void" else self._scalar(ret, f"{where}, return")
        params = [p.strip() for p in params.split(",")]
        args = [] if params in ([""], ["void"]) else [self._param(p, where) for p in params]
        self.functions[name] = (res, args)

    def _struct(self, body, name, where):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            m = re.fullmatch(r"(.*?)(\**)\s*(\w+)", first, re.S)
            if not m or not m.group(1).strip():
                raise HeaderError(f"{where}: cannot read field '{decl}'")
            base = m.group(1)
            for stars, field in [m.group(2, 3)] + [
                    re.fullmatch(r"(\**)\s*(.*)", p, re.S).groups() for p in more]:
                if not re.fullmatch(r"\w+", field):
                    raise HeaderError(f"{where}: cannot read field '{decl}'")
                fields.append((field, _POINTER if stars else
                               self._scalar(base, f"{where}, field '{field}'")))
        self.structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        self._opaque.add(name)

    def read(self, text, header):
        text = re.sub(r"/\*.*?\*/", " ", text.replace("\\\n", " "), flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for name, value in _DEFINE.findall(text):
            if value:  # the include guards have none
                try:
                    self.constants[name] = _constant(value)
                except (ValueError, SyntaxError):
                    raise HeaderError(f"{header}: #define {name} {value}: not an integer "
                                      "expression") from None
        text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
        for body, name in _STRUCT.findall(text):
            self._struct(body, name, f"{header}: struct {name}")
        text = re.sub(r'extern\s+"C"\s*\{', " ", _STRUCT.sub(" ", text))
        for stmt in filter(None, (s.strip(" \t\n}") for s in text.split(";"))):
            where = f"{header}: '{' '.join(stmt.split())}'"
            m = re.fullmatch(r"typedef\s+(.*?)(\w+)", stmt, re.S)
            if m:
                ctype, name = m.group(1).strip(), m.group(2)
                if re.fullmatch(r"struct\s+\w+", ctype):
                    self._opaque.add(name)  # only ever passed by pointer
                else:
                    self._types[name] = _POINTER if "*" in ctype else self._scalar(ctype, where)
                continue
            m = re.fullmatch(r"(.*?)\b(pn2(?:cpu)?_\w+)\s*\((.*)\)", stmt, re.S)
            if not m:
                raise HeaderError(f"{where}: not a typedef, a struct or a pn2_* prototype")
            self._function(m.group(1), m.group(2), m.group(3), f"{header}: {m.group(2)}")


def load(include_dir):
    """The Abi of the headers in `include_dir`."""
    abi = Abi()
    for h in HEADERS:
        path = os.path.join(include_dir, h)
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: the Python binding of libpn2hip.so is derived from the "
                "headers in include/ next to the package (a source checkout has them).")
        with open(path) as f:
            abi.read(f.read(), h)
    return abi
