"""The term text format of tests/host_harness/nif_driver.c (and of fake_print in
tests/nif_stub/fake_erl_nif.c), encoded and decoded.

    atom            name, or 'any text'      Atom("name")  (true / false are atoms too)
    integer, float  -12, 0.5                 int, float
    binary          <<hex>>                  bytes
    tuple, list     {a,b}  [a,b]  [a|t]      tuple, list, Improper(items, tail)
    map             #{k=>v}                  dict
    reference, pid  &N  @N                   Ref(N), Pid(N)
    resource        %type:serial             Res(type, serial)   (printed by the driver only)
    a bound name    $name                    Var("name")         (read by the driver only)

badarg, the exception a NIF raises, is printed as the atom badarg."""
import re


class Atom(str):
    def __repr__(self):
        return "Atom(%s)" % str.__repr__(self)


class _Num:
    def __init__(self, n):
        self.n = int(n)

    def __eq__(self, o):
        return type(o) is type(self) and o.n == self.n

    def __hash__(self):
        return hash((type(self).__name__, self.n))

    def __repr__(self):
        return "%s(%d)" % (type(self).__name__, self.n)


class Ref(_Num):
    pass


class Pid(_Num):
    pass


class Var:
    def __init__(self, name):
        self.name = name

    def __eq__(self, o):
        return isinstance(o, Var) and o.name == self.name

    def __hash__(self):
        return hash(("Var", self.name))

    def __repr__(self):
        return "Var(%r)" % self.name


class Res:
    def __init__(self, type_, serial):
        self.type, self.serial = type_, int(serial)

    def __eq__(self, o):
        return isinstance(o, Res) and (o.type, o.serial) == (self.type, self.serial)

    def __hash__(self):
        return hash((self.type, self.serial))

    def __repr__(self):
        return "Res(%r, %d)" % (self.type, self.serial)


class Improper:
    def __init__(self, items, tail):
        self.items, self.tail = list(items), tail

    def __eq__(self, o):
        return isinstance(o, Improper) and (o.items, o.tail) == (self.items, self.tail)

    def __repr__(self):
        return "Improper(%r, %r)" % (self.items, self.tail)


TRUE, FALSE, OK, ERROR, BADARG, UNDEFINED, NONE = (Atom(a) for a in (
    "true", "false", "ok", "error", "badarg", "undefined", "none"))
_PLAIN = re.compile(r"[a-z][a-zA-Z0-9_@]*\Z")


def boolean(v):
    return TRUE if v else FALSE


def encode(t) -> str:
    if isinstance(t, Atom):
        if _PLAIN.match(t):
            return str(t)
        assert "'" not in t
        return "'%s'" % t
    if isinstance(t, bool):
        return "true" if t else "false"
    if isinstance(t, int):
        return str(t)
    if isinstance(t, float):
        s = repr(t)
        return s if any(c in s for c in ".en") else s + ".0"
    if isinstance(t, (bytes, bytearray)):
        return "<<%s>>" % bytes(t).hex()
    if isinstance(t, tuple):
        return "{%s}" % ",".join(encode(x) for x in t)
    if isinstance(t, list):
        return "[%s]" % ",".join(encode(x) for x in t)
    if isinstance(t, Improper):
        return "[%s|%s]" % (",".join(encode(x) for x in t.items), encode(t.tail))
    if isinstance(t, dict):
        return "#{%s}" % ",".join("%s=>%s" % (encode(k), encode(v)) for k, v in t.items())
    if isinstance(t, Ref):
        return "&%d" % t.n
    if isinstance(t, Pid):
        return "@%d" % t.n
    if isinstance(t, Var):
        return "$" + t.name
    if isinstance(t, Res):
        return "%%%s:%d" % (t.type, t.serial)
    raise TypeError("no term for %r" % (t,))


_TOK = re.compile(r"""
    (?P<bin><<(?P<hex>[0-9a-f]*)>>)
  | (?P<map>\#\{)
  | (?P<res>%(?P<rtype>[A-Za-z0-9_]+):(?P<rser>\d+))
  | (?P<ref>&(?P<refn>\d+))
  | (?P<pid>@(?P<pidn>\d+))
  | (?P<var>\$(?P<vname>[A-Za-z0-9_]+))
  | (?P<float>-?\d+(?:\.\d+(?:e[-+]?\d+)?|e[-+]?\d+)|-?inf|nan)
  | (?P<int>-?\d+)
  | (?P<atom>[a-z][a-zA-Z0-9_@]*)
  | (?P<qatom>'(?P<qname>[^']*)')
  | (?P<punct>=>|[{}\[\],|])
""", re.X)


def decode(s: str):
    t, at = _term(s, 0)
    assert s[at:].strip() == "", "trailing text: %r" % s[at:at + 40]
    return t


def _tok(s, at):
    while at < len(s) and s[at] in " \t":
        at += 1
    m = _TOK.match(s, at)
    assert m, "cannot read a term at %r" % s[at:at + 40]
    return m, m.end()


def _seq(s, at, closers):
    items = []
    m, nx = _tok(s, at)
    if m.group("punct") in closers:
        return items, m.group("punct"), nx
    while True:
        t, at = _term(s, at)
        items.append(t)
        m, at = _tok(s, at)
        p = m.group("punct")
        if p in closers:
            return items, p, at
        assert p == ",", "expected , at %r" % s[at:at + 40]


def _term(s, at):
    m, at = _tok(s, at)
    k = m.lastgroup
    if m.group("bin") is not None:
        return bytes.fromhex(m.group("hex")), at
    if m.group("map") is not None:
        d = {}
        m2, nx = _tok(s, at)
        if m2.group("punct") == "}":
            return d, nx
        while True:
            key, at = _term(s, at)
            m2, at = _tok(s, at)
            assert m2.group("punct") == "=>"
            d[key], at = _term(s, at)
            m2, at = _tok(s, at)
            if m2.group("punct") == "}":
                return d, at
            assert m2.group("punct") == ","
    if m.group("res") is not None:
        return Res(m.group("rtype"), m.group("rser")), at
    if m.group("ref") is not None:
        return Ref(m.group("refn")), at
    if m.group("pid") is not None:
        return Pid(m.group("pidn")), at
    if m.group("var") is not None:
        return Var(m.group("vname")), at
    if m.group("float") is not None:
        return float(m.group("float")), at
    if m.group("int") is not None:
        return int(m.group("int")), at
    if m.group("atom") is not None:
        return Atom(m.group("atom")), at
    if m.group("qatom") is not None:
        return Atom(m.group("qname")), at
    p = m.group("punct")
    if p == "{":
        items, _, at = _seq(s, at, ("}",))
        return tuple(items), at
    if p == "[":
        items, closer, at = _seq(s, at, ("]", "|"))
        if closer == "|":
            tail, at = _term(s, at)
            m2, at = _tok(s, at)
            assert m2.group("punct") == "]"
            return Improper(items, tail), at
        return items, at
    raise AssertionError("unexpected %r (%s)" % (p, k))
