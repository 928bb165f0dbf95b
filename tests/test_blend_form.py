"""CPU test of the blend's launch forms (web-splat_amd/csrc/blend_form.h): which kernel a request becomes.  A wrong dispatch can
draw a right image (the coverage form with a null alpha pointer draws what the plain form draws), so the mapping itself is
checked here: a few lines of C++ against the header (plain C++, no HIP), compiled as the product and as the experimental build,
enumerate the whole request space; the expected outcome of every request is the table below, written from the launcher's four
rule copies as they stood before blend_form.h merged them (launch_blend / launch_blend_shape in raster.hip)."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-splat_amd", "csrc")

OK, INVALID, UNSUPPORTED, STATE = 0, -1, -4, -5  # ws_status (include/websplat.h)
K_BLEND, K_STRICT, K_Q, K_ASYNC = 0, 1, 2, 3     # BlendKernel
NONE, ALPHA, Z = 0, 1, 2                         # BlendAux
LOAD, OCCLUDE = 1, 2                             # BlendComp bits

# k_blend kernels in the built libraries, by build.  Checked against the libraries themselves below (one host launch stub per
# instantiated kernel: nm web-splat_amd/lib{,_exp}/libwebsplat_hip.so | grep -c __device_stub__k_blendI); 45 plain (18 + 9 capture
# + 18 exact cut), 36 with planes, 108 composite, 1 timing; the experimental build adds 18 LDS-DMA forms.
K_BLEND_KERNELS = {"product": 190, "experimental": 208}

# The request space: every value the launcher looks at, one invalid value per enumerated dimension included.
SPACE = dict(
    format=(0, 1, 2, 7), shape=((2, 2), (4, 2), (4, 4), (2, 4)), multi=(0, 1), split=(0, 1), capture=(0, 1), timing=(0, 1), exact=(0, 1),
    dma=(0, 1), async_staging=(0, 1), aux=(NONE, ALPHA, Z), has_z=(0, 1), comp=(0, LOAD, OCCLUDE, LOAD | OCCLUDE), variant=(0, 1, 2, 3))
ANY_COMP = (LOAD, OCCLUDE, LOAD | OCCLUDE)
NOT_PRODUCTION = ("capture", "timing", "dma", "exact", "async_staging")  # what launch_blend_shape refused planes / composite under


def k_blend(**kw):
    """An accepted request's k_blend form: format, shape and tiles-per-workgroup follow the request unless stated."""
    return dict(dict(kernel=K_BLEND, format="=format", qw="=qw", qh="=qh", multi="=multi", capture=0, dma=0, timing=0, exact=0, aux=NONE,
                     comp=0), **kw)


def other(kernel, comp=0):
    return dict(kernel=kernel, format="=format", qw=0, qh=0, multi=0, capture=0, dma=0, timing=0, exact=0, aux=NONE, comp=comp)


def rules(experimental):
    """(condition, outcome) in the order the parent's launcher tested them; the first whose condition holds decides.  A condition
    names request fields and the values (one, or a tuple) they must have; an outcome is an error code or the form launched."""
    r = [
        # launch_blend
        (dict(aux=Z, has_z=0), STATE),
        (dict(aux=(ALPHA, Z), variant=(1, 2, 3)), UNSUPPORTED),
        (dict(comp=(OCCLUDE, LOAD | OCCLUDE), has_z=0), STATE),
        (dict(comp=ANY_COMP, variant=(1, 3)), UNSUPPORTED),
        (dict(variant=2, format=7), INVALID),
        (dict(variant=2, comp=ANY_COMP), other(K_STRICT, comp=LOAD)),
        (dict(variant=2), other(K_STRICT)),
    ]
    r += [(dict(variant=1, format=7), INVALID), (dict(variant=1), other(K_Q))] if experimental else [(dict(variant=1), UNSUPPORTED)]
    r += [(dict(shape=((2, 4),)), INVALID)]
    # launch_blend_shape: the composite, then the auxiliary planes
    r += [({"comp": ANY_COMP, flag: 1}, UNSUPPORTED) for flag in NOT_PRODUCTION]
    r += [(dict(comp=ANY_COMP, format=7), INVALID),
          (dict(comp=ANY_COMP, aux=Z), k_blend(aux=Z, comp="=comp")),
          (dict(comp=ANY_COMP), k_blend(aux=ALPHA, comp="=comp"))]
    r += [({"aux": (ALPHA, Z), flag: 1}, UNSUPPORTED) for flag in NOT_PRODUCTION]
    r += [(dict(aux=(ALPHA, Z), format=7), INVALID), (dict(aux=(ALPHA, Z)), k_blend(aux="=aux"))]
    # ... the timing build
    r += [(dict(timing=1, shape=((2, 2), (4, 2))), UNSUPPORTED),
          (dict(timing=1, format=(0, 1, 7)), UNSUPPORTED),  # (rgba32float, 2, only)
          (dict(timing=1, capture=1), UNSUPPORTED), (dict(timing=1, multi=1), UNSUPPORTED), (dict(timing=1, dma=1), UNSUPPORTED),
          (dict(timing=1), k_blend(timing=1))]
    # ... barrier-free staging and LDS-DMA staging: experimental build only
    if experimental:
        eligible = dict(async_staging=1, shape=((4, 4),), capture=0, multi=0, dma=0, split=0)
        r += [(dict(eligible, format=7), INVALID), (eligible, other(K_ASYNC))]
    else:
        r += [(dict(async_staging=1), UNSUPPORTED), (dict(dma=1), UNSUPPORTED)]
    r += [(dict(format=7), INVALID)]
    if experimental:
        r += [(dict(dma=1, capture=0), k_blend(dma=1))]
    r += [(dict(exact=1, capture=0), k_blend(exact=1)), (dict(capture=1), k_blend(capture=1, multi=1)), (dict(), k_blend())]
    return r


FORM_FIELDS = ("kernel", "format", "qw", "qh", "multi", "capture", "dma", "timing", "exact", "aux", "comp")


def expected(req, table):
    for cond, outcome in table:
        if all(req[k] in v if isinstance(v, tuple) else req[k] == v for k, v in cond.items()):
            if isinstance(outcome, int):
                return (outcome,)
            return (OK,) + tuple(req[v[1:]] if isinstance(v, str) else v for v in (outcome[f] for f in FORM_FIELDS))
    raise AssertionError("the rule table ends in a catch-all")


PROBE = r"""
#include <stdio.h>
#include "blend_form.h"
using namespace ws;
int main() {
    constexpr BlendFormTable table = blend_form_table();
    unsigned k_blend_forms = 0;
    for (unsigned i = 0; i < table.n; ++i) k_blend_forms += BlendForm::of(table.bits[i]).kernel == BLEND_K;
    printf("k_blend_forms %%u all_forms %%u\n", k_blend_forms, table.n);
    const int formats[] = {%(format)s}, shapes[][2] = {%(shape)s}, auxs[] = {%(aux)s}, comps[] = {%(comp)s}, variants[] = {%(variant)s};
    for (int format : formats) for (auto& sh : shapes) for (int multi = 0; multi < 2; ++multi) for (int split = 0; split < 2; ++split)
    for (int capture = 0; capture < 2; ++capture) for (int timing = 0; timing < 2; ++timing) for (int exact = 0; exact < 2; ++exact)
    for (int dma = 0; dma < 2; ++dma) for (int async = 0; async < 2; ++async) for (int aux : auxs) for (int has_z = 0; has_z < 2; ++has_z)
    for (int comp : comps) for (int variant : variants) {
        BlendRequest q{};
        q.format = format, q.qw = sh[0], q.qh = sh[1], q.multi = multi, q.split = split;
        q.mode.capture = capture, q.mode.timing = timing, q.mode.exact_cut = exact, q.mode.dma = dma, q.mode.async_staging = async;
        q.mode.variant = variant, q.aux = aux, q.has_z = has_z, q.comp = comp;
        const BlendChoice c = blend_form_of(q);
        const BlendForm f = c.form;
        if (c.rc) { printf("%%d\n", c.rc); continue; }
        if (!blend_form_legal(f) || BlendForm::of(f.bits()).bits() != f.bits()) { printf("illegal form accepted\n"); return 1; }
        printf("0 %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", f.kernel, f.format, f.qw, f.qh, f.multi, f.capture, f.dma, f.timing, f.exact, f.aux, f.comp);
    }
    return 0;
}
"""


def _braces(values):
    return ", ".join("{%d, %d}" % v if isinstance(v, tuple) else str(v) for v in values)


@pytest.mark.parametrize("build", ["product", "experimental"])
def test_every_request_maps_to_the_parents_kernel_or_error(build, tmp_path):
    assert list(SPACE)[:2] == ["format", "shape"] and all(SPACE[k] == (0, 1) for k in ("multi", "split", "capture", "timing", "exact", "dma",
                                                                                       "async_staging", "has_z"))
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE % {k: _braces(SPACE[k]) for k in ("format", "shape", "aux", "comp", "variant")})
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include")] +
                   (["-DWS_EXPERIMENTAL"] if build == "experimental" else []) + [str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    # (a) as many legal k_blend forms as the library has k_blend kernels
    counts = dict(zip(out[0].split()[::2], map(int, out[0].split()[1::2])))
    assert counts["k_blend_forms"] == K_BLEND_KERNELS[build]
    assert counts["all_forms"] == K_BLEND_KERNELS[build] + (6 + 3 + 3 if build == "experimental" else 6)  # + k_blend_strict, k_blend_q, k_blend2
    lib = os.path.join(ROOT, "web-splat_amd", "lib" if build == "product" else "lib_exp", "libwebsplat_hip.so")
    stubs = set(re.findall(r"\S*__device_stub__k_blendI\S*", subprocess.run(["nm", lib], capture_output=True, text=True, check=True).stdout))
    assert len(stubs) == K_BLEND_KERNELS[build]
    # (b) request by request: the parent's error code, or the parent's kernel
    table = rules(build == "experimental")
    names = list(SPACE)
    got = [tuple(map(int, line.split())) for line in out[1:]]
    n = accepted = 0
    for values, g in zip(itertools.product(*SPACE.values()), got):
        req = dict(zip(names, values))
        req["qw"], req["qh"] = req["shape"]
        e = expected(req, table)
        assert g == e, (req, "got", g, "expected", e)
        n += 1
        accepted += g[0] == OK
    assert n == len(got) == 4 * 4 * 2 ** 8 * 3 * 4 * 4
    # every legal form is reached by some request (the dispatcher instantiates nothing that cannot be launched)
    assert len({g[1:] for g in got if g[0] == OK}) == counts["all_forms"]
    assert 0 < accepted < n
