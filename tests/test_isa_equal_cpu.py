"""scripts/prof/isa_equal.py: how it splits a compiler's assembly text into symbols and what it
normalises before comparing, on a canned snippet (no compile, no GPU)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("_isa_equal", os.path.join(ROOT, "scripts", "prof", "isa_equal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel(name, body, vgprs=4):
    return (f"\t.protected\t{name} ; -- Begin function {name}\n"
            f"\t.globl\t{name}\n"
            "\t.p2align\t8\n"
            f"\t.type\t{name},@function\n"
            f"{name}:\n"
            f"{body}"
            "\ts_endpgm\n"
            "\t.section\t.rodata,\"a\",@progbits\n"
            f"\t.amdhsa_kernel {name}\n"
            f"\t\t.amdhsa_next_free_vgpr {vgprs}\n"
            "\t.end_amdhsa_kernel\n"
            "\t.text\n"
            f"\t.set {name}.num_vgpr, {vgprs}\n"
            f"; NumVgprs: {vgprs}\n")


def _file(kernels, cuid):
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"
            "\t.text\n" + "".join(kernels) +
            f"\t.type\t__hip_cuid_{cuid},@object\n"
            f"__hip_cuid_{cuid}:\n"
            "\t.amdgpu_metadata\n"
            "amdhsa.kernels: []\n"
            "\t.end_amdgpu_metadata\n")


A = _kernel("_Z1av", "\tv_mov_b32_e32 v0, 0\n")
B = _kernel("_Z1bv", "\tv_mov_b32_e32 v1, 1\n")


def test_split_symbols():
    t = _tool()
    parts, kernels = t.split_symbols(_file([A, B], "0123abcd"))
    assert list(parts) == [t.HEAD, "_Z1av", "_Z1bv", t.TAIL]
    assert kernels == {"_Z1av", "_Z1bv"}
    # a symbol's text: the directives that name it, code, descriptor and resource comments
    assert "v_mov_b32_e32 v0, 0" in parts["_Z1av"] and ".amdhsa_next_free_vgpr 4" in parts["_Z1av"]
    assert "; NumVgprs: 4" in parts["_Z1av"] and "v_mov_b32_e32 v1, 1" not in parts["_Z1av"]
    assert parts["_Z1av"].startswith("\t.protected\t_Z1av") and parts["_Z1av"].endswith("; NumVgprs: 4")
    assert parts["_Z1bv"].startswith("\t.protected\t_Z1bv") and "_Z1bv" not in parts["_Z1av"]
    assert parts[t.HEAD] == "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.text"
    assert parts[t.TAIL].startswith("\t.type\t__hip_cuid_0123abcd,@object") and "amdhsa.kernels" in parts[t.TAIL]
    assert "\n".join(parts.values()) == _file([A, B], "0123abcd").rstrip("\n")  # nothing dropped


def test_only_the_cuid_is_normalised():
    t = _tool()
    assert t.compare(_file([A, B], "0123abcd"), _file([A, B], "fedc9876")) == (2, 2, [])
    assert t.normalise("x __hip_cuid_0123abcd y") == "x __hip_cuid_ y"
    spaced = _file([A, B], "0123abcd").replace("v0, 0", "v0,  0")  # any other change of text counts
    assert t.compare(_file([A, B], "0123abcd"), spaced)[2] == ["_Z1av"]


def test_differences_are_named_per_symbol():
    t = _tool()
    ref = _file([A, B], "0123abcd")
    code = _file([A, _kernel("_Z1bv", "\tv_mov_b32_e32 v1, 2\n")], "fedc9876")
    assert t.compare(ref, code) == (2, 2, ["_Z1bv"])
    budget = _file([A, _kernel("_Z1bv", "\tv_mov_b32_e32 v1, 1\n", vgprs=8)], "fedc9876")
    assert t.compare(ref, budget) == (2, 2, ["_Z1bv"])
    # a symbol one side lacks: named, and it alone (its leading directives are its own text)
    assert t.compare(ref, _file([A], "fedc9876")) == (2, 2, ["_Z1bv"])
    assert t.compare(ref, ref.replace("amdhsa.kernels: []", "amdhsa.kernels: [x]"))[2] == [t.TAIL]


def test_symbol_order_does_not_matter():
    """Two files that define the same symbols in another order (template instantiations reordered)
    are equal; a real difference is still named, and only that symbol."""
    t = _tool()
    ref = _file([A, B], "0123abcd")
    assert t.compare(ref, _file([B, A], "fedc9876")) == (2, 2, [])
    swapped = _file([_kernel("_Z1bv", "\tv_mov_b32_e32 v1, 2\n"), A], "fedc9876")
    assert t.compare(ref, swapped) == (2, 2, ["_Z1bv"])
    # comdat sections: the .section line in front of the .protected line names the symbol too
    sa = "\t.section\t.text._Z1av,\"axG\",@progbits,_Z1av,comdat\n" + A
    sb = "\t.section\t.text._Z1bv,\"axG\",@progbits,_Z1bv,comdat\n" + B
    assert t.compare(_file([sa, sb], "0123abcd"), _file([sb, sa], "fedc9876")) == (2, 2, [])
    parts, _ = t.split_symbols(_file([sa, sb], "0123abcd"))
    assert parts["_Z1bv"].startswith("\t.section\t.text._Z1bv") and "_Z1bv" not in parts["_Z1av"]
