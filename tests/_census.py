"""The compiled kernels by name (CPU only): each mangled gfx950 kernel symbol of the built library, spelt as
yalps_tableau_info's `launched=` spells the kernel it launched.

The symbols are plain Itanium manglings of templates in the unnamed namespace, e.g.
`_ZN12_GLOBAL__N_111wide_kernelILi1024ELi1ELb1ELb0EEEvNS_4DescEiiiPKd` = wide_kernel<1024, 1, true, false>.  Integer
template arguments are written as they are, in template order; a bool argument is written as the switch that selects it
(nothing when false), except PANEL of stream3_kernel, which is `panel` or `direct`.  pivot_kernel's fourth argument (the
unroll depth D) follows from <T, J, R> and is left out, as the host's table does."""
import re

_HEAD = re.compile(r"^_ZN12_GLOBAL__N_1(\d+)")
_ARG = re.compile(r"L([ib])(n?\d+)E")

# kernel -> the spelling of its bool template arguments, in template order (a pair: (when true, when false))
_BOOLS = {
    "resident_kernel": ("lds", "tag"),
    "stream_kernel": ("check",),
    "stream2_kernel": ("nt",),
    "stream3_kernel": ("nt", "check", ("panel", "direct")),
    "sweep_kernel": ("check", "nt"),
    "dshard_kernel": ("nt", "panel"),
    "dshard_sweep_kernel": ("nt",),
    "wide_kernel": ("inplace", "nt"),
    "small_kernel": ("check",),
    "batch_kernel": ("lds",),
}
# kernels whose trailing integer arguments are implied by the others
_DROP_INTS = {"pivot_kernel": 1}


def parse(symbol):
    """(kernel name, [template arguments: int or bool]) of a mangled kernel symbol."""
    m = _HEAD.match(symbol)
    if not m:
        raise ValueError("not a kernel of the unnamed namespace: %r" % symbol)
    n, at = int(m.group(1)), m.end()
    name = symbol[at:at + n]
    at += n
    args = []
    if symbol[at:at + 1] == "I":
        at += 1
        while symbol[at:at + 1] != "E":
            a = _ARG.match(symbol, at)
            if not a:
                raise ValueError("unexpected template argument in %r at %d" % (symbol, at))
            v = int(a.group(2).replace("n", "-"))
            args.append(bool(v) if a.group(1) == "b" else v)
            at = a.end()
    return name, args


def spelling(symbol):
    """The `launched=` spelling of a mangled kernel symbol."""
    name, args = parse(symbol)
    ints = [a for a in args if not isinstance(a, bool)]
    bools = [a for a in args if isinstance(a, bool)]
    if _DROP_INTS.get(name):
        ints = ints[:len(ints) - _DROP_INTS[name]]
    flags = _BOOLS.get(name, ())
    if len(flags) != len(bools):
        raise ValueError("%s: %d bool template arguments, spelling known for %d" % (name, len(bools), len(flags)))
    parts = [str(i) for i in ints]
    for f, b in zip(flags, bools):
        on, off = f if isinstance(f, tuple) else (f, "")
        if (on if b else off):
            parts.append(on if b else off)
    return name + ("<%s>" % ",".join(parts) if parts else "")


def census(symbols):
    """{spelling: symbol}; two symbols with one spelling are an error."""
    out = {}
    for s in symbols:
        k = spelling(s)
        if k in out:
            raise ValueError("%s and %s both spell %s" % (out[k], s, k))
        out[k] = s
    return out
