"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports
every symbol include/gymrl.h declares, and the ctypes binding (gymrl_amd/_lib.py: one SIGNATURES line per entry
point, one Structure per struct) says what the header says; no compute is launched (no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _header_text():
    hdr = open(os.path.join(ROOT, "include", "gymrl.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.sub(r"#ifdef GYMRL_PROF_BUILD.*?#endif", "", hdr, flags=re.S)      # probe-build-only declarations


def _declared_symbols():
    return sorted(set(re.findall(r"\b(gymrl_[a-z0-9_]+)\s*\(", _header_text())))


def _c_type(decl, what):
    """'const float* x[4]' -> (('float', 1, '4'), 'x'): base type, pointer depth, array length (0: not an array)."""
    m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?", decl.strip(), flags=re.S)
    assert m and m.group(1).strip(), f"{what}: cannot parse `{' '.join(decl.split())}`"
    base = " ".join(t for t in m.group(1).replace("*", " ").split() if t != "const")
    return (base, m.group(1).count("*"), m.group(3) or 0), m.group(2)


def _parse_header():
    """include/gymrl.h as (functions, structs): name -> (return type, [parameter types]) in the header's order, and typedef
    name -> [(field, type)]; a type is (base, pointer depth, array length), a struct named by its tag reads as its typedef.
    Anything between the structs, enums and forward declarations that is not a prototype fails here, by name."""
    hdr = _header_text()
    consts = {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\s*$", hdr, flags=re.M)}
    hdr = re.sub(r"^\s*#.*$", "", hdr, flags=re.M)
    hdr = re.sub(r'extern\s+"C"\s*\{', "", hdr)
    structs, tags = {}, {}

    def take_struct(m):
        tag, body, name = m.groups()
        assert "{" not in body, f"struct {name}: nested braces"
        if tag:
            tags["struct " + tag] = name
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            (base, ptr, arr), fname = _c_type(first, f"struct {name}")
            fields.append((fname, (base, ptr, arr)))
            for extra in more:        # `double gamma, lam;`: the declarators after the first carry no base type
                (_, ptr2, arr2), fname2 = _c_type(base + " " + extra, f"struct {name}")
                fields.append((fname2, (base, ptr2, arr2)))
        structs[name] = []
        for fname, (base, ptr, arr) in fields:
            arr = consts.get(arr, arr)
            assert isinstance(arr, int) or arr.isdigit(), f"struct {name}.{fname}: unknown array length {arr}"
            structs[name].append((fname, (base, ptr, int(arr))))
        return ""

    hdr = re.sub(r"typedef\s+struct\s*(\w+)?\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, hdr, flags=re.S)
    hdr = re.sub(r"\benum\s*\{.*?\}\s*;", "", hdr, flags=re.S)
    hdr = re.sub(r"\bstruct\s+\w+\s*;", "", hdr)                                 # forward declarations
    functions = {}
    for decl in filter(None, (d.strip() for d in hdr.split(";"))):
        if decl == "}":                                                           # closes extern "C"
            continue
        m = re.fullmatch(r"(.*?)\b(gymrl_\w+)\s*\((.*)\)", decl, flags=re.S)
        assert m, f"include/gymrl.h: cannot parse the declaration `{' '.join(decl.split())}`"
        ret, name, params = m.groups()
        assert name not in functions, f"{name} is declared twice"
        types = [_c_type(ret + " _", name)[0]]
        types += [] if params.strip() == "void" else [_c_type(p, name)[0] for p in params.split(",")]
        for base, ptr, arr in types:
            assert not arr and ptr <= 1, f"{name}: array or pointer-to-pointer in a prototype"
        types = [(tags.get(base, base), ptr, arr) for base, ptr, arr in types]
        functions[name] = (types[0], types[1:])
    return functions, structs


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "unsigned int": ctypes.c_uint,
            "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "unsigned long long": ctypes.c_ulonglong,
            "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
# typedef structs of the header the binding never builds: name -> why (none today)
_NOT_MIRRORED = {}


def _mirrors():
    from gymrl_amd import _lib
    classes = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    for c in classes:
        assert getattr(c, "_c_name_", None), f"_lib.{c.__name__} does not name its header struct (_c_name_)"
    by_name = {c._c_name_: c for c in classes}
    assert len(by_name) == len(classes), "two mirrors name one header struct"
    return by_name


def _agrees(ct, htype, mirrors):
    """Does the ctypes type say what the header type says?  Scalars and structs by value: the exact type.  A pointer:
    c_void_p, or POINTER of the exact pointee (void has none).  An array: the length and the element."""
    base, ptr, arr = htype
    if arr:
        return issubclass(ct, ctypes.Array) and ct._length_ == arr and _agrees(ct._type_, (base, ptr, 0), mirrors)
    exact = _SCALARS.get(base) or mirrors.get(base)
    if ptr:
        return ct is ctypes.c_void_p or (exact is not None and ct is ctypes.POINTER(exact))
    return exact is not None and ct is exact


def _spell(ct):
    return getattr(ct, "__name__", repr(ct))


def test_library_exports_every_declared_symbol():
    from gymrl_amd import _lib
    L = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gymrl.h but not exported"
    assert sorted(_lib.SYMBOLS) == declared, "gymrl_amd/_lib.py SYMBOLS out of sync with include/gymrl.h"
    assert L.gymrl_abi_version() == 4 == _lib.ABI_VERSION
    # the product library carries no diagnostic switches (timing-only kernel variants live in the probe build)
    assert not hasattr(L, "gymrl_gemm_config")


def test_signature_table_says_what_the_header_says():
    """Every SIGNATURES line against its prototype: arity, return type, every parameter."""
    from gymrl_amd import _lib
    functions, _ = _parse_header()
    mirrors = _mirrors()
    assert list(_lib.SIGNATURES) == list(functions), "gymrl_amd/_lib.py SIGNATURES: not the header's names in the header's order"
    assert _lib.SYMBOLS == list(_lib.SIGNATURES)
    for name, (ret, params) in functions.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert ret[1] == 0 and restype is _SCALARS[ret[0]], f"{name}: returns {ret[0]}, the table says {_spell(restype)}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table"
        for i, (ct, htype) in enumerate(zip(argtypes, params)):
            assert _agrees(ct, htype, mirrors), f"{name}: parameter {i} is {htype[0]}{'*' * htype[1]}, the table says {_spell(ct)}"


def test_struct_mirrors_say_what_the_header_says():
    """Every ctypes.Structure of _lib.py against its typedef struct, field by field: name, order, type, array length."""
    from gymrl_amd import _lib
    _, structs = _parse_header()
    mirrors = _mirrors()
    assert len(structs) >= 19
    assert set(mirrors) <= set(structs), f"mirrors of no header struct: {sorted(set(mirrors) - set(structs))}"
    assert set(structs) - set(mirrors) == set(_NOT_MIRRORED), "a header struct without a mirror is listed in _NOT_MIRRORED, with a reason"
    for cname, cls in mirrors.items():
        fields = structs[cname]
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], f"{cname} ({cls.__name__}): field names or their order differ"
        for (fname, ct), (_, htype) in zip(cls._fields_, fields):
            assert _agrees(ct, htype, mirrors), (f"{cname}.{fname} is {htype[0]}{'*' * htype[1]}{'[%d]' % htype[2] if htype[2] else ''}, "
                                                 f"{cls.__name__} says {_spell(ct)}")
    # the layouts the library itself reports (the size queries stay exported)
    L = _lib.lib()
    assert L.gymrl_mlprnn_params_bytes() == ctypes.sizeof(_lib.MlprnnParams) == 28 * 8
    assert (L.gymrl_sac_args_bytes(0), L.gymrl_sac_args_bytes(1)) == (ctypes.sizeof(_lib.SacActArgs), ctypes.sizeof(_lib.SacUpdateArgs))
    assert (L.gymrl_rainbow_args_bytes(0), L.gymrl_rainbow_args_bytes(1)) == (ctypes.sizeof(_lib.RainbowActArgs),
                                                                               ctypes.sizeof(_lib.RainbowUpdateArgs))


def test_lib_applies_the_table_and_refuses_a_wrong_type():
    """lib() types every exported function, so a wrongly typed argument raises before it reaches the library."""
    from gymrl_amd import _lib
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    null = ctypes.c_void_p(None)
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_env_obs_dim(ctypes.c_int64(0))                                  # int64 object for an int
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_gae_workspace_bytes(2048, 4096.0)                               # float for an int
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_soft_update(null, null, 8, ctypes.c_float(0.005), null)         # float object for a double
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_soft_update(null, null, ctypes.c_int(8), 0.005, null)           # int object for an int64_t
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_rollout_lunar(ctypes.byref(_lib.MlpDesc()), ctypes.byref(_lib.MlpDesc()), null)   # another struct's pointer
    with pytest.raises(ctypes.ArgumentError):
        L.gymrl_gru_seq_fwd(null, null, null, null, (ctypes.c_int64 * 2)(), 1, 2, 16, null, null, null)   # i64 host array for i32
    with pytest.raises(TypeError):
        L.gymrl_env_state_bytes(0)                                              # a missing argument
    assert L.gymrl_soft_update(null, null, 8, 0.005, null) == -22               # plain Python scalars convert


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """_lib.lib() compares the library's ABI version with the one this front-end was written against."""
    from gymrl_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", 999)
    with pytest.raises(RuntimeError, match="ABI version"):
        _lib.lib()
    monkeypatch.setattr(_lib, "ABI_VERSION", 4)
    assert _lib.lib().gymrl_abi_version() == 4


def test_size_queries_need_no_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    assert L.gymrl_env_obs_dim(0) == 4 and L.gymrl_env_obs_dim(1) == 3 and L.gymrl_env_obs_dim(2) == 8
    assert L.gymrl_env_act_dim(0) == 2 and L.gymrl_env_act_dim(2) == 4
    assert L.gymrl_env_max_steps(0) == 500 and L.gymrl_env_max_steps(1) == 200 and L.gymrl_env_max_steps(2) == 1000
    assert L.gymrl_env_state_bytes(0, 4096) > 0
    assert L.gymrl_gae_workspace_bytes(2048, 4096) > 0
    assert L.gymrl_env_obs_dim(99) == -22          # EINVAL, like the header says


def test_bad_arguments_return_einval_without_gpu():
    from gymrl_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(None)
    assert L.gymrl_gae(null, null, null, null, 4, 4, ctypes.c_double(0.99), ctypes.c_double(0.95), null, null,
                       null, 0, null, null) == -22
    assert L.gymrl_soft_update(null, null, ctypes.c_int64(8), ctypes.c_double(0.005), null) == -22


def test_new_entry_points_validate_arguments_without_gpu():
    """Argument validation happens before any HIP call: NULL pointers, unsupported shapes and
    inconsistent descriptors return -EINVAL (22) on a machine with no GPU at all."""
    from gymrl_amd import _lib
    L = _lib.lib()
    null, i64, dbl = ctypes.c_void_p(None), ctypes.c_int64, ctypes.c_double
    assert L.gymrl_mlp_packed_floats(4, 8) == 1 * 4 * 256 and L.gymrl_mlp_packed_floats(256, 256) == 16 * 16 * 256
    assert L.gymrl_mlp_packed_floats(0, 8) == 0
    assert L.gymrl_mlp_pack(null, 4, 8, null, null) == -22
    desc = _lib.MlpDesc()
    desc.n_stages = 0
    fake = ctypes.c_void_p(256)                       # never dereferenced: validation fails first
    assert L.gymrl_mlp_forward(fake, 16, 8, ctypes.byref(desc), null) == -22          # no stages
    desc.n_stages = 1
    desc.stage[0].W, desc.stage[0].in_dim, desc.stage[0].out_dim = 256, 8, 4
    desc.stage[0].src, desc.stage[0].dst, desc.stage[0].act = -1, 1, 7
    assert L.gymrl_mlp_forward(fake, 16, 8, ctypes.byref(desc), null) == -22          # unknown activation
    desc.stage[0].act, desc.stage[0].dst = 0, -1
    assert L.gymrl_mlp_forward(fake, 16, 8, ctypes.byref(desc), null) == -22          # dst == -1 without `out`
    assert L.gymrl_mlp_forward(fake, 16, 100, ctypes.byref(desc), null) == -22         # input wider than supported
    assert L.gymrl_mlp_train_workspace_bytes(256, 8, 4) >= 4 * 1024 * 9 * 256
    assert L.gymrl_linear_tanh_smallk(fake, fake, null, i64(8), 8, 48, fake, null) == -22     # C not a power of two
    assert L.gymrl_linear_tanh_smallk(fake, fake, null, i64(8), 5, 64, fake, null) == -22     # unsupported input width
    assert L.gymrl_tanh_inplace(fake, i64(6), null, 0, null) == -22                            # n % 4 != 0
    assert L.gymrl_heads_bwd(fake, fake, fake, i64(8), 64, 3, fake, fake, fake, fake, fake, fake, fake, fake, 0, null,
                             fake, null) == -22                                                # A not in {2, 4}
    assert L.gymrl_heads_fwd_tanh(null, i64(8), 64, 4, null, fake, null, fake, null, fake, fake, 1, null) == -22
    args = _lib.RolloutLunarArgs()
    assert L.gymrl_rollout_lunar(ctypes.byref(args), ctypes.byref(desc), null) == -22          # NULL slabs
    # the fused off-policy steps: NULL / empty argument blocks are refused before any launch
    act, upd = _lib.SacActArgs(), _lib.SacUpdateArgs()
    assert L.gymrl_sac_act_step(ctypes.byref(act), null) == -22 and L.gymrl_sac_update(ctypes.byref(upd), null) == -22
    # empty work is a no-op that returns 0 without launching anything
    assert L.gymrl_tanh_inplace(fake, i64(0), null, 0, null) == 0
    assert L.gymrl_linear_tanh_smallk(fake, fake, null, i64(0), 8, 64, fake, null) == 0


def test_mhc_entry_points_validate_arguments_without_gpu():
    """PPO-full's mHC kernels: shapes outside what a kernel is written for are -EINVAL before any HIP call."""
    from gymrl_amd import _lib
    L = _lib.lib()
    null, f32 = ctypes.c_void_p(None), ctypes.c_float
    fake = ctypes.c_void_p(256)                       # never dereferenced: validation fails first
    gates = lambda n, D, stats: L.gymrl_mhc_gates(fake, fake, fake, fake, fake, 8, n, D, 10, fake, fake, fake, fake, stats, null)  # noqa: E731
    assert gates(3, 128, null) == -22                  # branches: 2 or 4
    assert gates(2, 6, null) == -22                    # D % 4
    assert gates(4, 64, fake) == -22                   # the read-out sums exist for n = 2, n * D in (256, 512) only
    assert gates(2, 64, fake) == -22
    assert L.gymrl_mhc_gates(fake, fake, fake, fake, fake, 0, 2, 128, 10, fake, fake, fake, fake, fake, null) == 0   # empty batch
    assert L.gymrl_mhc_combine(fake, fake, fake, fake, 8, 2, 128, 1, fake, null) == -22          # act: none or SiLU
    assert L.gymrl_mhc_combine_bwd(fake, fake, fake, fake, fake, 8, 2, 128, 2, fake, fake, fake, null, null) == -22
    assert L.gymrl_mhc_combine_bwd(fake, fake, fake, fake, fake, 0, 2, 128, 5, fake, fake, fake, null, null) == 0    # d_h may be NULL
    assert L.gymrl_mhc_read_bwd(fake, fake, fake, 8, 3, 128, fake, null, 0, null) == -22
    bwd = lambda n, D, stats, ws: L.gymrl_mhc_gates_bwd(fake, fake, fake, fake, fake, fake, fake, stats, fake, fake, fake, null, null,  # noqa: E731
                                                        8, n, D, fake, fake, fake, fake, fake, ws, null)
    assert bwd(4, 64, fake, fake) == -22 and bwd(2, 64, fake, fake) == -22 and bwd(2, 128, null, fake) == -22
    assert bwd(2, 128, fake, null) == -22              # workspace required
    assert L.gymrl_mhc_gates_bwd_workspace_bytes(2, 128) >= 512 * 2315 * 4
    assert L.gymrl_mhc_gates_bwd_workspace_bytes(2, 256) >= 2 * 512 * 2315 * 4
    assert L.gymrl_rmsnorm(fake, fake, 8, 128, 1, f32(1e-6), 3, fake, null) == -22
    assert L.gymrl_rmsnorm_bwd(fake, fake, fake, 8, 513, f32(1e-6), 0, fake, fake, fake, null) == -22      # D <= 512
    assert L.gymrl_rmsnorm_bwd(fake, fake, fake, 8, 128, f32(1e-6), 0, fake, fake, null, null) == -22      # workspace required
    assert L.gymrl_rmsnorm_bwd_workspace_bytes(256) >= 2048 * 256 * 4
    pol = _lib.MhcPolicy()
    assert L.gymrl_mhc_policy_forward(null, fake, 8, fake, fake, null) == -22
    # the packed operand image: its size is a function of the sub-block count; pack refuses NULL / misaligned / incomplete inputs
    assert L.gymrl_mhc_policy_image_floats(4) == 4 * (128 * 128 + 256 * 8) + 2 * 256 * 128 and L.gymrl_mhc_policy_image_floats(9) == 0
    assert L.gymrl_mhc_policy_pack(null, fake, null) == -22 and L.gymrl_mhc_policy_pack(ctypes.byref(pol), null, null) == -22
    assert L.gymrl_mhc_policy_pack(ctypes.byref(pol), ctypes.c_void_p(260), null) == -22        # image not 16-byte aligned
    assert L.gymrl_mhc_policy_pack(ctypes.byref(pol), fake, null) == -22                        # NULL parameters
    pol.obs_dim, pol.n_sub, pol.n_act, pol.sk_it = 8, 2, 4, 10
    assert L.gymrl_mhc_policy_forward(ctypes.byref(pol), fake, 8, fake, fake, null) == -22       # NULL parameters
    pol.in_w = pol.in_b = pol.final_norm_w = 256
    assert L.gymrl_mhc_policy_forward(ctypes.byref(pol), fake, 8, fake, fake, null) == -22       # NULL sub-block parameters
    pol.n_sub, pol.obs_dim = 9, 8
    assert L.gymrl_mhc_policy_forward(ctypes.byref(pol), fake, 8, fake, fake, null) == -22       # more than 8 sub-blocks
    pol.n_sub, pol.obs_dim = 0, 17
    assert L.gymrl_mhc_policy_forward(ctypes.byref(pol), fake, 8, fake, fake, null) == -22       # more than 16 observations
    # the weight gradient's slice count follows the shape (64 x 64 blocks from 16384 rows on): the workspace query says so
    small, big = L.gymrl_lin_workspace_bytes(8192, 128, 128, 1), L.gymrl_lin_workspace_bytes(262144, 128, 128, 1)
    assert small == 32 * (128 * 128 + 128) * 4 and big == 512 * (128 * 128 + 128) * 4


def test_linear_geometry_is_host_only_and_refuses_what_the_entries_refuse():
    """gymrl_linear_geometry walks the entries' dispatch without a launch: one round up to row_groups * rows_per_round rows,
    a row-group count that stops growing there, and -EINVAL for the shapes gymrl_linear_fwd / _bwd_input / _bwd_input_add refuse."""
    from gymrl_amd import _lib, ops
    L = _lib.lib()
    g, r = ctypes.c_int(0), ctypes.c_int(0)
    for kind, shapes in ((0, [(256, 256), (256, 512), (128, 128), (128, 256), (64, 64), (64, 128)]),
                         (1, [(256, 256), (256, 512), (128, 256), (128, 128), (64, 128), (64, 64)]), (2, [(128, 256)])):
        for K, N in shapes:
            rg_max, rpr = ops.linear_geometry(kind, 1 << 40, K, N)
            assert rpr in (128, 256) and rg_max >= 8
            assert ops.linear_geometry(kind, 1, K, N) == (1, rpr)
            assert ops.linear_geometry(kind, 5 * rpr + 1, K, N) == (6, rpr)              # one row group per started round-of-one
            assert ops.linear_geometry(kind, rg_max * rpr, K, N) == (rg_max, rpr)        # the largest single-round call
            assert ops.linear_geometry(kind, rg_max * rpr + 1, K, N) == (rg_max, rpr)    # one row more: a second round
    assert L.gymrl_linear_geometry(0, 100, 256, 128, g, r) == -22                        # no such forward
    assert L.gymrl_linear_geometry(1, 100, 96, 96, g, r) == -22
    assert L.gymrl_linear_geometry(2, 100, 256, 256, g, r) == -22                        # bwd_input_add: (N, K) = (256, 128) only
    assert L.gymrl_linear_geometry(3, 100, 256, 256, g, r) == -22                        # unknown kind
    assert L.gymrl_linear_geometry(0, 0, 256, 256, g, r) == -22 and L.gymrl_linear_geometry(0, -4, 256, 256, g, r) == -22
    assert L.gymrl_linear_geometry(0, 100, 256, 256, None, r) == -22 and L.gymrl_linear_geometry(0, 100, 256, 256, g, None) == -22


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from gymrl_amd import ops
    x = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gae(x, x, x.to(torch.uint8), x[0], 0.99, 0.95, variant=0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "gymrl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                for needle in ("import oracle", "from oracle", "libgymrl_oracle", "oracle/", "orc_"):
                    assert needle not in src, f"{f} uses the oracle ({needle})"
