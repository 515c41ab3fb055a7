"""A strict reader of the small subset of C that include/splat_hip.h is written in.

parse(text) returns a Header: integer constants (#define and enumerators), structs as ordered (name, Type) fields and prototypes as
(restype, [argument Types]).  Whatever lies outside the subset -- an unknown type, a bit-field, a union, a function pointer, a
#define that is no integer, a struct used before it is declared -- raises CDeclError with the line: the reader understands a
declaration or refuses it, it never guesses.  _native.py builds the ctypes binding from this model, so the header is the only
place where the C ABI is declared.
"""
import ast
import re
from collections import namedtuple

# base: a SCALARS name, "void" or a struct name; array: the length of `name[n]` or None; host: marked with HOST_MARKER
Type = namedtuple("Type", "base const pointer array host")
Header = namedtuple("Header", "constants structs functions")

SCALARS = ("int8_t", "int16_t", "int32_t", "int64_t", "uint8_t", "uint16_t", "uint32_t", "uint64_t", "float", "double", "size_t", "int",
           "char")
HOST_MARKER = "SGR_HOST"        # an empty macro in front of a declaration: the pointer addresses host memory
_TOKEN = re.compile(r"[A-Za-z_]\w*|\d\w*|<<|>>|[{}()\[\];,*=+\-:]|(\S)")       # group 1: what is no token
_IDENT = re.compile(r"[A-Za-z_]\w*")
_OPS = {ast.Add: int.__add__, ast.Sub: int.__sub__, ast.Mult: int.__mul__, ast.LShift: int.__lshift__, ast.RShift: int.__rshift__}


class CDeclError(ValueError):
    pass


class _Reader:
    def __init__(self, text, name):
        self.name, self.constants, self.structs, self.functions = name, {}, {}, {}
        self.toks, self.pos = self._tokens(self._preprocess(text)), 0

    def fail(self, line, what):
        raise CDeclError(f"{self.name}:{line}: {what}")

    def value(self, expr, line):
        """An integer expression of literals, earlier constants, + - * ( ) and shifts."""
        def ev(n):
            if isinstance(n, ast.Constant) and type(n.value) is int:
                return n.value
            if isinstance(n, ast.Name) and n.id in self.constants:
                return self.constants[n.id]
            if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
                return -ev(n.operand)
            if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
                return _OPS[type(n.op)](ev(n.left), ev(n.right))
            raise ValueError
        try:
            return ev(ast.parse(expr.strip(), mode="eval").body)
        except (SyntaxError, ValueError):
            self.fail(line, f"'{expr.strip()}' is not an integer expression of literals and earlier constants")

    def _preprocess(self, text):
        """Comments and directives blanked (the line count kept), #define taken in, the inactive side of #ifdef / #ifndef dropped."""
        text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
        lines, defined, active = re.sub(r"//[^\n]*", "", text).split("\n"), set(), []
        for i, raw in enumerate(lines):
            s, ln = raw.strip(), i + 1
            if s.endswith("\\"):
                self.fail(ln, "line continuations are not supported")
            if not s.startswith("#"):
                if not all(active):
                    lines[i] = ""
                continue
            lines[i] = ""
            m = re.fullmatch(r"#\s*(\w+)\s*(.*)", s)
            word, rest = m.groups() if m else ("", "")
            if word in ("ifdef", "ifndef") and re.fullmatch(r"\w+", rest):
                active.append((rest in defined or rest in self.constants) == (word == "ifdef"))
            elif word == "endif" and active:
                active.pop()
            elif not all(active):
                continue
            elif word == "include":
                pass
            elif word == "define" and re.fullmatch(r"[A-Za-z_]\w*", rest):
                defined.add(rest)           # the include guard, HOST_MARKER
            elif word == "define" and re.match(r"[A-Za-z_]\w*\s", rest):
                name, expr = rest.split(None, 1)
                if name in self.constants:
                    self.fail(ln, f"{name} is defined twice")
                self.constants[name] = self.value(expr, ln)
            else:
                self.fail(ln, f"unsupported directive '{s}'")
        if active:
            self.fail(len(lines), "#endif is missing")
        return "\n".join(lines)

    def _tokens(self, text):
        toks = []
        for ln, line in enumerate(text.split("\n"), 1):
            for m in _TOKEN.finditer(line):
                if m.group(1):
                    self.fail(ln, f"unexpected character {m.group(1)!r}")
                toks.append((m.group(), ln))
        return toks + [("<end of file>", ln)]

    # ---- the parser: one token of look-ahead -----------------------------------------------------------------------------------
    def peek(self):
        return self.toks[self.pos][0]

    def line(self):
        return self.toks[self.pos][1]

    def accept(self, tok):
        if self.peek() == tok:
            self.pos += 1
            return True
        return False

    def expect(self, tok):
        if not self.accept(tok):
            self.fail(self.line(), f"expected '{tok}', found '{self.peek()}'")

    def ident(self, what):
        tok, ln = self.toks[self.pos]
        if not _IDENT.fullmatch(tok):
            self.fail(ln, f"expected {what}, found '{tok}'")
        self.pos += 1
        return tok

    def expr_until(self, *stops):
        ln, start = self.line(), self.pos
        while self.peek() not in stops:
            if self.peek() in (";", "{", "<end of file>"):
                self.fail(ln, f"expected '{stops[0]}', found '{self.peek()}'")
            self.pos += 1
        return self.value(" ".join(t for t, _ in self.toks[start:self.pos]), ln)

    def type_(self):
        ln = self.line()
        host, const = self.accept(HOST_MARKER), self.accept("const")
        base = self.ident("a type")
        if base in ("struct", "union", "enum"):
            self.fail(ln, f"'{base}' inside a declaration is not supported (typedef it first)")
        if base != "void" and base not in SCALARS and base not in self.structs:
            self.fail(ln, f"unknown type '{base}'")
        pointer = self.accept("*")
        if self.peek() in ("*", "const"):
            self.fail(ln, "only `[const] T*` pointers are supported")
        if self.peek() == "(":
            self.fail(ln, "function pointers are not supported")
        return Type(base, const, pointer, None, host)

    def declarator(self, t, parameter):
        """`name` or `name[n]` after the type t -> (name, Type)."""
        ln = self.line()
        name = self.ident("a name")
        if self.accept("["):
            t = t._replace(array=self.expr_until("]"))
            self.expect("]")
            if t.array < 1 or self.peek() == "[":
                self.fail(ln, f"{name}: only one array dimension of a positive length is supported")
        if self.peek() == ":":
            self.fail(ln, f"{name}: bit-fields are not supported")
        indirect = t.pointer or (parameter and t.array is not None)       # an array parameter is a pointer
        if t.base == "void" and not indirect:
            self.fail(ln, f"{name}: void by value")
        if t.host and not (indirect and t.base in SCALARS):
            self.fail(ln, f"{name}: {HOST_MARKER} marks pointers to scalars only")
        return name, t

    def enum(self, ln):
        if self.peek() != "{":
            self.ident("a tag")
        self.expect("{")
        value = -1
        while not self.accept("}"):
            eln, name = self.line(), self.ident("an enumerator")
            value = self.expr_until(",", "}") if self.accept("=") else value + 1
            if name in self.constants:
                self.fail(eln, f"{name} is defined twice")
            self.constants[name] = value
            if self.peek() != "}":
                self.expect(",")
        self.ident("the enum's name")
        self.expect(";")

    def struct(self, ln):
        tag = self.ident("a tag")
        self.expect("{")
        fields = []
        while not self.accept("}"):
            t = self.type_()
            fields.append(self.declarator(t, False))
            while self.accept(","):
                fields.append(self.declarator(t, False))
            self.expect(";")
        if not fields or len({n for n, _ in fields}) != len(fields):
            self.fail(ln, f"{tag}: no field, or a field name twice")
        if self.ident("the struct's name") != tag or tag in self.structs:
            self.fail(ln, f"expected `typedef struct {tag} {{ ... }} {tag};`, once")
        self.expect(";")
        self.structs[tag] = fields

    def prototype(self):
        ln = self.line()
        res = self.type_()
        if res.host:
            self.fail(ln, f"{HOST_MARKER} does not apply to a return type")
        name, args = self.ident("a function name"), []
        if name in self.functions:
            self.fail(ln, f"{name} is declared twice")
        self.expect("(")
        if self.toks[self.pos][0] == "void" and self.toks[self.pos + 1][0] == ")":
            self.pos += 1
        else:
            args.append(self.declarator(self.type_(), True)[1])
            while self.accept(","):
                args.append(self.declarator(self.type_(), True)[1])
        self.expect(")")
        self.expect(";")
        self.functions[name] = (res, args)

    def run(self):
        while self.peek() != "<end of file>":
            ln = self.line()
            if not self.accept("typedef"):
                self.prototype()
            elif self.accept("enum"):
                self.enum(ln)
            elif self.accept("struct"):
                self.struct(ln)
            else:
                self.fail(ln, f"typedef of '{self.peek()}': only `typedef struct` and `typedef enum` are supported")
        return Header(self.constants, self.structs, self.functions)


def parse(text, name="splat_hip.h"):
    return _Reader(text, name).run()
