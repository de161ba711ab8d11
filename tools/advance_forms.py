"""Which launch is this?  The form word of a wf_advance kernel (csrc/rt_still.h kForm*) from its name, for the tools that read traces, statistics and assembly.

One kernel template carries every form -- `rtk::wf_advance<FORM, Extra...>`: demangled `void rtk::wf_advance<5u, rtk::TexScene>(rtk::Scene, ...)`, mangled
`_ZN3rtk10wf_advanceILj5EJNS_8TexSceneEEEEv...` -- where 21 named kernels stood before; the traces and tables committed under profiles/ spell those, so both are known
here and nowhere else.  form_of(name) -> the word, or None for another kernel."""
import re

BITS = {"stats": 1 << 0, "first": 1 << 1, "tex": 1 << 2, "anim": 1 << 3, "list": 1 << 4, "fill": 1 << 5, "resume": 1 << 6, "lights": 1 << 7, "soft": 1 << 8,
        "lens": 1 << 9, "close": 1 << 10, "shutter": 1 << 11, "sky": 1 << 12, "sample": 1 << 13, "emit": 1 << 14, "fresnel": 1 << 15, "gloss": 1 << 16, "tint": 1 << 17}
_B = BITS
# the names the forms had as kernels of their own (demangled, spaces dropped)
OLD = {"wf_advance<false,false>": 0, "wf_advance<true,false>": _B["stats"], "wf_advance<false,true>": _B["first"], "wf_advance<true,true>": _B["first"] | _B["stats"],
       "wf_advance_tex<false>": _B["tex"], "wf_advance_tex<true>": _B["tex"] | _B["stats"], "wf_advance_fill": _B["fill"], "wf_advance_resume": _B["resume"],
       "wf_advance_lights": _B["lights"], "wf_advance_tex_lights": _B["tex"] | _B["lights"], "wf_advance_soft": _B["soft"], "wf_advance_tex_soft": _B["tex"] | _B["soft"],
       "wf_advance_lens": _B["first"] | _B["lens"], "wf_advance_anim<false>": _B["anim"], "wf_advance_anim<true>": _B["first"] | _B["anim"],
       "wf_advance_tex_anim": _B["tex"] | _B["anim"], "wf_advance_close<false>": _B["close"], "wf_advance_close<true>": _B["close"] | _B["stats"],
       "wf_advance_list<false>": _B["list"], "wf_advance_list<true>": _B["first"] | _B["list"], "wf_advance_list_tex": _B["tex"] | _B["list"]}
# the forms that came after the one template and never had a kernel name of their own: the four of the shutter
LATER = [_B["first"] | _B["shutter"], _B["first"] | _B["lens"] | _B["shutter"], _B["shutter"], _B["tex"] | _B["shutter"]]
FORMS = sorted(set(OLD.values()) | set(LATER))                         # the 25 built for a scene without an environment (tests/test_shutter_forms.py holds the number)
# ... and the four of the environment (kFormSky: the later launches of a chain under a map)
SKY_FORMS = sorted([_B["sky"], _B["tex"] | _B["sky"], _B["soft"] | _B["sky"], _B["tex"] | _B["soft"] | _B["sky"]])
ALL_FORMS = sorted(FORMS + SKY_FORMS)                                  # the 29 that are built without sky sampling (tests/test_sky_forms.py holds the number)
# ... and the two of sky sampling (kFormSkySample: the later launches of a chain whose shadow rays may go to the environment; any lights take the soft route)
SKY_SAMPLE_FORMS = sorted([_B["soft"] | _B["sky"] | _B["sample"], _B["tex"] | _B["soft"] | _B["sky"] | _B["sample"]])
# ... and the two of the emissive meshes (kFormEmit: the later launches of a chain in whose scene a mesh emits; any lights take the soft route)
EMISSION_FORMS = sorted([_B["soft"] | _B["emit"], _B["tex"] | _B["soft"] | _B["emit"]])
# ... and the four of the Fresnel dielectrics (kFormFresnel: the later launches of a chain in whose scene an object is effectively flagged; a light list or a radius takes the soft route)
FRESNEL_FORMS = sorted([_B["fresnel"], _B["tex"] | _B["fresnel"], _B["soft"] | _B["fresnel"], _B["tex"] | _B["soft"] | _B["fresnel"]])
# ... and the four of the rough mirrors (kFormGloss: the later launches of a chain in whose scene a mirror has an effective roughness; a light list or a radius takes the soft route)
GLOSS_FORMS = sorted([_B["gloss"], _B["tex"] | _B["gloss"], _B["soft"] | _B["gloss"], _B["tex"] | _B["soft"] | _B["gloss"]])
# ... and the four of the tinted mirrors and glass (kFormTint, always beside kFormGloss: the later launches of a chain in whose scene an object is effectively tinted, a mirror of it rough or not)
TINT_FORMS = sorted([g | _B["tint"] for g in GLOSS_FORMS])


def form(*names):
    """form("tex", "anim") -> the word"""
    return sum(BITS[n] for n in names)


def form_of(kernel_name):
    name = kernel_name.replace(" ", "")
    m = re.search(r"wf_advance<(?:\(unsignedint\))?(\d+)u?[,>]", name) or re.search(r"_ZN3rtk10wf_advanceILj(\d+)E", name)
    if m:
        return int(m.group(1))
    m = re.search(r"wf_advance\w*(?:<(?:true|false)(?:,(?:true|false))?>)?", name)
    return OLD.get(m.group(0)) if m else None


def mangled_prefix(f):
    """what the assembly label of form f begins with (the extras and the signature follow)"""
    return "_ZN3rtk10wf_advanceILj%dEJ" % f


def describe(f):
    return "wf_advance<" + (" | ".join(n for n, b in BITS.items() if f & b) or "0") + ">"
