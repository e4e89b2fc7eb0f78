"""Strict reader of include/usseg.h: the ctypes structs, prototypes and integer constants of the C ABI, from the one place that declares them.

It understands exactly what the header uses - ``#define NAME <integer>``, enums with explicit values, ``typedef struct X { ... } X;`` (several
declarators per line, arrays sized by literals or earlier constants, nested structs, pointer fields) and function declarations - and raises
``AbiError`` naming the line for anything else.  It never guesses: a wrong guess loads cleanly and hands a kernel the wrong bytes.

Pointers: a pointer to a declared struct is a typed ``POINTER`` (as a parameter: unless its name ends in ``_dev``, a device table the host never
dereferences); every other pointer is ``c_void_p``; a ``const char*`` return is ``c_char_p``.
"""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}
_TOKEN = re.compile(r"\s*([A-Za-z_]\w*|-?(?:0[xX][0-9a-fA-F]+|\d+)|[*\[\],(){}=+-])")
_INT = re.compile(r"-?(0[xX][0-9a-fA-F]+|\d+)")
_NAME = re.compile(r"[A-Za-z_]\w*")


class AbiError(ValueError):
    pass


class Abi:
    def __init__(self):
        self.consts = {}    # #define and enum names -> int
        self.types = {}     # typedef names -> ctypes type (structs included)
        self.structs = {}   # struct name -> ctypes.Structure subclass, in declaration order
        self.protos = {}    # function name -> (restype, [argtypes])


def parse(text: str, origin: str = "usseg.h") -> Abi:
    abi = Abi()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: re.sub(r"[^\n]", " ", m.group()), text, flags=re.S)

    def fail(off, why, what):
        raise AbiError(f"{origin}:{text.count(chr(10), 0, off) + 1}: {why}: {' '.join(what.split())!r}")

    def tokens(off, s):
        out, i = [], 0
        while s[i:].strip():
            m = _TOKEN.match(s, i)
            if not m:
                fail(off, f"unexpected character {s[i:].strip()[0]!r} in", s)
            out.append(m.group(1))
            i = m.end()
        return out

    def const(off, tok, decl):
        if _INT.fullmatch(tok):
            return int(tok, 0)
        if tok not in abi.consts:
            fail(off, f"{tok!r} is neither an integer nor an earlier constant in", decl)
        return abi.consts[tok]

    def const_expr(off, toks, decl):
        """an integer, a constant, or one + - of two of them (USSEG_SCHED_MAX_PIECES - 1)"""
        if len(toks) == 1:
            return const(off, toks[0], decl)
        if len(toks) == 3 and toks[1] in "+-":
            a, b = const(off, toks[0], decl), const(off, toks[2], decl)
            return a + b if toks[1] == "+" else a - b
        fail(off, f"array size {' '.join(toks)!r} is not an integer, a constant or a sum of two in", decl)

    def base_type(off, tok, decl):
        if tok in SCALARS or tok in abi.types or tok in ("void", "char"):
            return tok
        fail(off, f"unknown type {tok!r} in", decl)

    def declarator(off, toks, decl):
        """``** name [a][b]`` -> (stars, name, dims)"""
        stars = 0
        while toks and toks[0] == "*":
            stars, toks = stars + 1, toks[1:]
        if not toks or not _NAME.fullmatch(toks[0]):
            fail(off, "cannot split the declaration", decl)
        name, toks, dims = toks[0], toks[1:], []
        while toks:
            if toks[0] != "[" or "]" not in toks:
                fail(off, "cannot split the declaration", decl)
            close = toks.index("]")
            dims.append(const_expr(off, toks[1:close], decl))
            toks = toks[close + 1:]
        return stars, name, dims

    def declaration(off, text, single=False, decl=None):
        """``const T *a, b[4]`` -> (T, [(stars, name, dims), ...]), or (T, stars, name, dims) of a single declarator; const carries no layout.
        ``decl``: the declaration that ``text`` is a part of, for the error message."""
        decl = decl or text
        toks = [t for t in tokens(off, text) if t != "const"]
        if len(toks) < 2:
            fail(off, "cannot split the declaration", decl)
        base, rest, group, out = base_type(off, toks[0], decl), toks[1:], [], []
        for t in rest + [","]:
            if t == ",":
                out.append(declarator(off, group, decl))
                group = []
            else:
                group.append(t)
        if single and len(out) != 1:
            fail(off, "cannot split the declaration", decl)
        return (base, *out[0]) if single else (base, out)

    def value_type(off, base, decl):
        if base in ("void", "char"):
            fail(off, f"{base!r} by value in", decl)
        return SCALARS.get(base) or abi.types[base]

    def struct(off, name, body, body_off):
        fields, pos = [], 0
        for part in body.split(";")[:-1]:
            foff = body_off + pos + (len(part) - len(part.lstrip()))
            pos += len(part) + 1
            base, decls = declaration(foff, part)
            for stars, fname, dims in decls:
                if stars:
                    t = C.POINTER(abi.structs[base]) if stars == 1 and base in abi.structs else C.c_void_p
                else:
                    t = value_type(foff, base, part)
                for n in reversed(dims):
                    if n <= 0:
                        fail(foff, f"array size {n} in", part)
                    t = t * n
                fields.append((fname, t))
        if body.split(";")[-1].strip() or not fields:
            fail(off, "cannot split the declaration", f"struct {name} {{{body}}}")
        short = name[len("Usseg"):] if name.startswith("Usseg") else name
        abi.structs[name] = abi.types[name] = type(short, (C.Structure,), {"_fields_": fields, "__doc__": f"{name} of {origin}"})

    def enum(off, body, decl):
        for item in body.split(","):
            if not item.strip():
                continue
            toks = tokens(off, item)
            if len(toks) != 3 or toks[1] != "=" or not _NAME.fullmatch(toks[0]) or not _INT.fullmatch(toks[2]):
                fail(off, f"enumerator {' '.join(item.split())!r} is not NAME = <integer> in", decl)
            abi.consts[toks[0]] = int(toks[2], 0)

    def function(off, decl):
        m = re.fullmatch(r"\s*([^()]*?)\s*\(([^()]*)\)\s*", decl)
        if not m or "{" in decl:
            fail(off, "cannot split the declaration", decl)
        base, stars, name, dims = declaration(off, m.group(1), single=True, decl=decl)
        if dims or stars > 1 or (stars == 1 and base != "char"):
            fail(off, "unsupported return type in", decl)
        res = C.c_char_p if stars else value_type(off, base, decl)
        args = []
        if m.group(2).strip() != "void":
            for p in m.group(2).split(","):
                pbase, pstars, pname, pdims = declaration(off, p, single=True, decl=decl)
                if pdims:
                    fail(off, "array parameter in", decl)
                if not pstars:
                    args.append(value_type(off, pbase, decl))
                elif pstars == 1 and pbase in abi.structs and not pname.endswith("_dev"):
                    args.append(C.POINTER(abi.structs[pbase]))
                else:
                    args.append(C.c_void_p)
        if name in abi.protos:
            fail(off, "declared twice", decl)
        abi.protos[name] = (res, args)

    # the preprocessor lines: the include guard, includes, the extern "C" bracket and integer defines; blanked so that offsets stay
    lines, guard, skipping, nxt = text.split("\n"), [], False, 0          # guard: [NAME] inside the include guard, [NAME, None] after its #endif
    for i, line in enumerate(lines):
        s, off, nxt = line.strip(), nxt, nxt + len(line) + 1
        if skipping:
            if s == "#endif":
                skipping = False
            elif s not in ("", 'extern "C" {', "}"):
                fail(off, "unexpected text under #ifdef __cplusplus", line)
            lines[i] = ""
        elif s.startswith("#"):
            d = s[1:].split()
            if s.endswith("\\"):
                fail(off, "continued preprocessor line", line)
            if d[:2] == ["ifdef", "__cplusplus"] and len(d) == 2:
                skipping = True
            elif d[0] == "ifndef" and len(d) == 2 and not guard:
                guard.append(d[1])
            elif d[0] == "endif" and len(d) == 1 and guard and guard[-1]:
                guard.append(None)
            elif d[0] == "include" and len(d) == 2:
                pass
            elif d[0] == "define" and len(d) == 2 and guard and d[1] == guard[0]:
                pass
            elif d[0] == "define" and len(d) == 3 and _NAME.fullmatch(d[1]) and _INT.fullmatch(d[2]):
                abi.consts[d[1]] = int(d[2], 0)
            else:
                fail(off, "unsupported preprocessor line", line)
            lines[i] = ""
    body = "\n".join(lines)
    if skipping or (guard and guard[-1] is not None):
        fail(len(body), "unterminated #if", lines[-1])

    # the declarations: every ';' outside braces ends one
    depth, start = 0, 0
    for i, ch in enumerate(body):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            decl, start = body[start:i], i + 1
            off = i - len(decl.lstrip())
            m = re.fullmatch(r"\s*typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)\s*", decl, flags=re.S)
            if m:
                if m.group(1) != m.group(3) or m.group(1) in abi.types:
                    fail(off, "struct tag and typedef name differ, or the name is taken, in", decl)
                struct(off, m.group(1), m.group(2), off + decl.lstrip().index("{") + 1)
                continue
            m = re.fullmatch(r"\s*(?:typedef\s+enum\s+(\w+)|enum)\s*\{([^{}]*)\}\s*(\w*)\s*", decl, flags=re.S)
            if m:
                if (m.group(1) or "") != m.group(3):
                    fail(off, "enum tag and typedef name differ in", decl)
                enum(off, m.group(2), decl)
                continue
            if re.match(r"\s*typedef\b", decl):
                base, stars, name, dims = declaration(off, decl.split("typedef", 1)[1], single=True, decl=decl)
                if dims or name in abi.types:
                    fail(off, "unsupported typedef", decl)
                abi.types[name] = C.c_void_p if stars else value_type(off, base, decl)
                continue
            function(off, decl)
    rest = body[start:].lstrip()
    if depth or rest:
        fail(len(body) - len(rest), "truncated declaration", rest[:200])
    return abi
