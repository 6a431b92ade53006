"""CPU (no GPU): the C ABI loads and exports what include/rba_hip.h declares; host logic (config reader, arch /
checkpoint contract, error behaviour of the op wrappers without a device); multi-process metric exchange on gloo."""
import ctypes
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rba_amd import arch as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.findall(r"\b(?:int|int64_t)\s+(rba_\w+)\s*\(", src)


def test_cabi_exports_every_declared_symbol():
    from rba_amd import _lib
    names = header_functions()
    assert len(names) >= 8 and "rba_reduce_f32" in names and "rba_ms_deform_attn_fwd_f32" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rba_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes signatures out of sync with the header"
    assert _lib.load().rba_hip_version() >= 100


def header_source():
    """include/rba_hip.h without comments -- also the /* ... */ inside argument lists"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)


def binding_type(decl):
    """the ctypes type the binding gives one C argument / field declaration: any pointer travels as void*, scalars by their own type"""
    if "*" in decl:
        return ctypes.c_void_p
    *base, _name = decl.replace("const ", " ").split()
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[" ".join(base)]


def test_cabi_signatures_match_the_header_argument_by_argument():
    """_lib.SIGNATURES is typed by hand beside the header: a c_int for an int64_t, or a missing argument, passes every test without a device and corrupts
    the call on one.  Every prototype, every argument, the return types and the one struct are compared here."""
    from rba_amd import _lib
    src = header_source()
    protos = {name: (ret, [] if args.strip() == "void" else args.split(","))
              for ret, name, args in re.findall(r"\b(int|int64_t)\s+(rba_\w+)\s*\(([^()]*)\)\s*;", src)}
    assert set(protos) == set(header_functions()) == set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, (ret, args) in protos.items():
        assert [binding_type(a) for a in args] == _lib.SIGNATURES[name], f"{name}: argtypes differ from the header"
        assert (ret == "int64_t") == name.endswith(("_bytes", "_elems")), f"{name}: return type {ret}"
        assert getattr(lib, name).restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*rba_token_linear_problem\s*;", src, flags=re.S).group(1)
    fields = [(f.split()[-1].lstrip("*"), binding_type(f)) for f in body.split(";") if f.strip()]
    assert fields == _lib.TokenLinearProblem._fields_


def test_product_library_has_no_writable_state_and_the_knobs_build_does():
    """include/rba_hip.h: "no mutable global state except the launch-geometry hint".  The tuning knobs of csrc/knobs.h are compile-time constants in
    librba_hip.so (no data symbol named rba_*) and exported ints only in librba_hip_knobs.so, which tests / tools load to select kernel variants."""
    import subprocess
    from rba_amd import _lib
    from rba_amd._lib import RbaHipError

    def data_symbols(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return sorted(ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "BDbdGgSsCc" and ln.split()[2].startswith("rba_"))

    assert data_symbols(_lib.LIB_PATH) == []
    knobs = data_symbols(_lib.KNOBS_LIB_PATH)
    assert {"rba_k1_up4_variant", "rba_k2_variant", "rba_k4_variant", "rba_k5_wpe", "rba_k6_rs", "rba_k6_ks", "rba_skinny_variant", "rba_token_rt"} <= set(knobs)
    with pytest.raises(RbaHipError, match="compile-time constant"):
        _lib.knob("rba_k6_rs")
    with _lib.use_library(_lib.KNOBS_LIB_PATH) as lib:
        assert _lib.load() is lib and _lib.knob("rba_k6_rs").value == 0 and lib.rba_hip_version() == _lib.EXPECTED_ABI
        for n in header_functions():
            assert hasattr(lib, n)
    assert _lib.load() is not lib


def test_ops_have_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.rba_reduce(torch.zeros(2, 4, 4), torch.zeros(2, 19))
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_forward(torch.zeros(1, 4, 2, 4), torch.ones(1, 2, dtype=torch.long), torch.zeros(1, dtype=torch.long),
                                   torch.zeros(1, 4, 2, 1, 2, 2), torch.zeros(1, 4, 2, 1, 2))
    with pytest.raises(RbaHipError):
        ops.resample_bilinear(torch.zeros(1, 2, 2), (4, 4))
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.linear(torch.zeros(4, 32), torch.nn.Linear(32, 128))
    for fn, args in ((ops.split_weight, (torch.zeros(128, 32),)), (ops.gaussian_blur, (torch.zeros(16, 16),)),
                     (ops.ood_components, (torch.zeros(16, 16), 0.0)), (ops.group_norm_nhwc, (torch.zeros(1, 8, 32), 4, torch.ones(32), torch.zeros(32))),
                     (ops.conv3x3_weight, (torch.zeros(128, 32, 3, 3),))):
        with pytest.raises(RbaHipError):
            fn(*args)


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under rba_amd/ may import it"""
    for root, _, files in os.walk(os.path.join(REPO, "rba_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(root, f)


def test_relative_position_index_matches_reference(golden):
    from rba_amd.modeling.backbone.swin import relative_position_index
    g = golden("g3_swin_parts")
    assert np.array_equal(relative_position_index(6).numpy(), g["wa_sd.relative_position_index"])


@pytest.mark.parametrize("name", ["g4_tiny1_60x90", "g4_tiny3_60x90", "g4_tiny1_dh_60x90", "g5_swin_b_1dl_1024x2048", "g5_swin_b_9dl_720x1280",
                                  "g5_swin_l_1dl_1024x2048"])
def test_model_state_dict_contract(golden, name):
    """our module tree has exactly the reference's state-dict keys and shapes (the model_final.pth contract) -- the toy
    architectures and the released ones (Swin-B 1dl / 9dl, Swin-L 1dl: MODEL_ZOO.md:54-69)"""
    from rba_amd.maskformer_model import MaskFormer
    g = golden(name)
    m = MaskFormer(A.ARCHS[str(g["arch"])])
    sd = m.state_dict()
    assert sorted(sd) == list(g["sd_keys"])
    assert [",".join(map(str, sd[k].shape)) for k in sorted(sd)] == list(g["sd_shapes"])


def test_checkpoint_loading(tmp_path):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS["tiny1"])
    sd = A.seeded_weights(a, 3)
    # .pth as Detectron2 writes it, DDP "module." prefix, extra criterion buffer
    pth = tmp_path / "model_final.pth"
    torch.save({"model": {"module." + k: v for k, v in sd.items()} | {"module.criterion.empty_weight": torch.ones(20)},
                "iteration": 7}, pth)
    m = load_checkpoint(MaskFormer(a), str(pth))
    k = "sem_seg_head.predictor.class_embed.bias"
    assert torch.equal(m.state_dict()[k], sd[k])
    # .pkl with numpy arrays (tools/convert-pretrained-swin-model-to-d2.py layout)
    pkl = tmp_path / "model_final.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "third_party", "matching_heuristics": True}, f)
    m2 = load_checkpoint(MaskFormer(a), str(pkl))
    assert torch.equal(m2.state_dict()[k], sd[k])
    # legacy names: static_query -> query_feat (decoder.py:237-258), pixel-decoder keys directly under the head (head.py:31-53)
    old = {}
    for kk, v in sd.items():
        kk = kk.replace("query_feat", "static_query")
        kk = kk.replace("sem_seg_head.pixel_decoder.", "sem_seg_head.")
        old[kk] = v
    m3 = load_checkpoint(MaskFormer(a), old)
    assert torch.equal(m3.state_dict()["sem_seg_head.predictor.query_feat.weight"], sd["sem_seg_head.predictor.query_feat.weight"])
    assert torch.equal(m3.state_dict()["sem_seg_head.pixel_decoder.mask_features.weight"],
                       sd["sem_seg_head.pixel_decoder.mask_features.weight"])
    # failures are loud
    bad = dict(sd)
    bad.pop(k)
    with pytest.raises(RuntimeError, match="missing"):
        load_checkpoint(MaskFormer(a), bad)
    bad = dict(sd)
    bad[k] = torch.zeros(7)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        load_checkpoint(MaskFormer(a), bad)


def test_config_reader(tmp_path):
    from rba_amd.config import load_cfg
    base = tmp_path / "base.yaml"
    base.write_text("MODEL:\n  SWIN:\n    EMBED_DIM: 128\n    DEPTHS: [2, 2, 18, 2]\n    NUM_HEADS: [4, 8, 16, 32]\n    WINDOW_SIZE: 12\n"
                    "  MASK_FORMER:\n    DEC_LAYERS: 10\nINPUT:\n  MIN_SIZE_TRAIN: !!python/object/apply:eval [\"[1, 2]\"]\n")
    child = tmp_path / "child.yaml"
    child.write_text("_BASE_: base.yaml\nMODEL:\n  MASK_FORMER:\n    DEC_LAYERS: 2\n  SEM_SEG_HEAD:\n"
                     "    DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES: [res5]\n")
    cfg = load_cfg(str(child), ["OUTPUT_DIR", "output/"])
    assert cfg.OUTPUT_DIR == "output/" and cfg.MODEL.SWIN.EMBED_DIM == 128 and cfg.MODEL.MASK_FORMER.DEC_LAYERS == 2
    assert A.arch_from_cfg(cfg) == A.complete(A.ARCHS["swin_b_1dl"])
    # unsupported features fail loudly instead of silently building something else
    cfg.MODEL.MASK_FORMER.PRE_NORM = True
    with pytest.raises(NotImplementedError):
        A.arch_from_cfg(cfg)


@pytest.mark.skipif(not os.path.isdir("/root/reference/ckpts"), reason="reference tree not present on this box")
def test_reference_ckpt_configs_parse():
    from rba_amd.config import load_cfg
    want = {"swin_b_1dl": "swin_b_1dl", "swin_b_1dl_rba_ood_coco": "swin_b_1dl", "swin_b_1dl_rba_ood_map_coco": "swin_b_1dl",
            "swin_l_1dl": "swin_l_1dl", "swin_l_1dl_rba_ood_map_coco": "swin_l_1dl"}
    for d, name in want.items():
        a = A.arch_from_cfg(load_cfg(f"/root/reference/ckpts/{d}/config.yaml"))
        inference_keys = ("panoptic_on", "open_panoptic", "object_mask_threshold", "overlap_threshold")
        want_a = A.complete(A.ARCHS[name])
        assert {k: v for k, v in a.items() if k not in inference_keys} == {k: v for k, v in want_a.items() if k not in inference_keys}, d
        # the released configs evaluate semantic inference only (their panoptic thresholds, 0.8 or the 0.0 default, are carried along)
        assert a["panoptic_on"] is False and a["object_mask_threshold"] in (0.0, 0.8) and a["overlap_threshold"] in (0.0, 0.8), d


def test_shard_indices():
    from rba_amd.distributed import shard_indices
    for n in (0, 1, 16, 17):
        for world in (1, 2, 8):
            parts = [shard_indices(n, r, world) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(n))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


_WORKER = r'''
import os, sys, json
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from rba_amd import distributed as D
from rba_amd.metrics import ood_metrics, select_labelled
rank, world, local = D.init_from_env("gloo")
aff = D.bind_rank_to_gpu_numa(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))     # no GPU here: the even split of the allowed CPUs by local rank
assert aff["bound"] and aff["cpus"] >= 1 and len(os.sched_getaffinity(0)) == aff["cpus"], aff
rng = np.random.RandomState(0)
n_img = int(sys.argv[2])
gts = rng.choice([0, 1, 255], size=(n_img, 40, 50), p=[0.85, 0.05, 0.10])
scores = (rng.randn(n_img, 40, 50) + 1.5 * (gts == 1)).astype(np.float32)
mine = D.shard_indices(n_img, rank, world)                      # ragged: 3 + 2 images (world 2), 2 + 2 + 2 + 1 x 5 (world 8)
s, y = select_labelled(torch.from_numpy(scores[mine]), torch.from_numpy(gts[mine]))
pooled = D.pooled_ood_metrics(s, y)
hist = D.histogram_ood_metrics(s, y)
single = ood_metrics(*select_labelled(torch.from_numpy(scores), torch.from_numpy(gts)))
# order of pooling differs from the single-process concatenation but the metrics are rank statistics: identical
ok = all(abs(pooled[k] - single[k]) < 1e-12 for k in single) and all(abs(hist[k] - single[k]) < 2e-3 for k in single)
g = D.all_gather_variable(torch.arange(rank + 2, dtype=torch.float32))
ok = ok and g.tolist() == [float(v) for r in range(world) for v in range(r + 2)]
print(json.dumps({"rank": rank, "ok": bool(ok), "pooled": pooled, "single": single, "hist": hist, "affinity": aff}), flush=True)
torch.distributed.destroy_process_group()
sys.exit(0 if ok else 1)
'''


@pytest.mark.parametrize("world,n_img,port", [(2, 5, 29611), (8, 11, 29627)])
def test_metric_exchange_gloo(tmp_path, world, n_img, port):
    """the pooled-metric exchange of rba_amd.distributed (sizes all_gather + padded all_gather_into_tensor, histogram all_reduce) under torch.distributed.run
    with 2 and with 8 ranks (gloo, CPU): ragged shards, pooled == single-process to 1e-12; every rank pins itself to its share of the CPUs first
    (bind_rank_to_gpu_numa -- here the no-NUMA-information fallback)."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script), REPO, str(n_img)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('"ok": true') == world


def test_rank_cpu_placement_follows_the_gpus_numa_node(tmp_path):
    """rba_amd.distributed.plan_rank_cpus / gpu_local_cpus / parse_cpulist: 8 GPUs on two sockets with SMT (GPU 0-3 -> node 0: CPUs 0-63,128-191; GPU 4-7 ->
    node 1) -- every rank gets a quarter of ITS node, disjoint from every other rank's, inside the cgroup's allowed set; no NUMA information -> even split."""
    from rba_amd import distributed as D
    assert D.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11] and D.parse_cpulist("") == []
    node = {0: D.parse_cpulist("0-63,128-191"), 1: D.parse_cpulist("64-127,192-255")}
    local = lambda r: node[r // 4]
    plans = [D.plan_rank_cpus(r, 8, local, range(256)) for r in range(8)]
    sets = [set(p[0]) for p in plans]
    assert all(len(s_) == 32 for s_ in sets) and len(set().union(*sets)) == 256
    assert all(sets[r] <= set(node[r // 4]) for r in range(8)) and "share 2/4" in plans[1][1]
    restricted = [D.plan_rank_cpus(r, 8, local, range(0, 96)) for r in range(8)]                 # a cgroup that only grants CPUs 0-95
    assert all(set(p[0]) <= set(range(96)) and p[0] for p in restricted)
    assert set(restricted[0][0]) <= set(node[0]) and set(restricted[5][0]) <= set(node[1])
    none = [D.plan_rank_cpus(r, 4, lambda r_: None, range(8)) for r in range(4)]
    assert [p[0] for p in none] == [[0, 1], [2, 3], [4, 5], [6, 7]] and "even split" in none[0][1]
    # sysfs reader on a fake tree
    class P:                                                                                          # noqa: N801
        pci_domain_id, pci_bus_id, pci_device_id = 0, 0xC1, 0
    d = tmp_path / "0000:c1:00.0"
    d.mkdir()
    (d / "local_cpulist").write_text("64-67\n")
    import unittest.mock as um
    with um.patch("torch.cuda.get_device_properties", return_value=P()):
        assert D.gpu_local_cpus(0, sysfs=str(tmp_path)) == [64, 65, 66, 67]
        assert D.gpu_local_cpus(0, sysfs=str(tmp_path / "missing")) is None
    assert D.bind_rank_to_gpu_numa(0, 1)["bound"] is False                                            # a single local rank is left alone


def test_bench_self_launch_refuses_without_devices():
    """`python bench.py --gpus 2` outside torchrun spawns its own ranks; with fewer visible devices than ranks it says so."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RBA_BENCH_SHARE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                       timeout=300)
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two devices visible: the launch would really run")
    assert r.returncode != 0 and "visible HIP device" in r.stderr


def test_dense_hybrid_config_flag(tmp_path):
    """MODEL.MASK_FORMER.DENSE_HYBRID_LOSS (config.py:220) switches the `ood_pred` head on; its keys join the state-dict contract"""
    import yaml
    from rba_amd.config import load_cfg
    cfg = {"MODEL": {"META_ARCHITECTURE": "MaskFormer", "BACKBONE": {"NAME": "D2SwinTransformer"},
                     "MASK_FORMER": {"DENSE_HYBRID_LOSS": True}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    a = A.arch_from_cfg(load_cfg(str(tmp_path / "config.yaml")))
    assert a["dense_hybrid"] is True
    keys = A.state_dict_shapes(a)
    assert "sem_seg_head.predictor.ood_pred.conv.weight" in keys and keys["sem_seg_head.predictor.ood_pred.conv.weight"][0] == (2, 256, 1, 1)
    assert "sem_seg_head.predictor.ood_pred.norm.running_var" in keys


def test_resnet50_config_and_state_dict_contract(tmp_path):
    """BASELINE config C1: maskformer2_R50_bs16_90k.yaml on Base-Cityscapes-SemanticSegmentation.yaml (build_resnet_backbone) parses
    to the ResNet-50 architecture, and the module tree has Detectron2's key layout (backbone.stem.conv1.{weight,norm.*},
    backbone.res{2..5}.{i}.{shortcut,conv1,conv2,conv3}.*)."""
    import yaml
    from rba_amd.config import load_cfg
    from rba_amd.maskformer_model import MaskFormer
    cfg = {"MODEL": {"META_ARCHITECTURE": "MaskFormer", "BACKBONE": {"NAME": "build_resnet_backbone", "FREEZE_AT": 0},
                     "RESNETS": {"DEPTH": 50, "STEM_OUT_CHANNELS": 64, "STRIDE_IN_1X1": False, "NORM": "SyncBN",
                                 "OUT_FEATURES": ["res2", "res3", "res4", "res5"]},
                     "SEM_SEG_HEAD": {"DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res5"]},
                     "MASK_FORMER": {"DEC_LAYERS": 2}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    a = A.arch_from_cfg(load_cfg(str(tmp_path / "config.yaml")))
    assert a["resnet"] == A.RESNET50 and a["dec_layers"] == 1 and a["enc_in"] == ["res5"]
    m = MaskFormer(a)
    sd = m.state_dict()
    shapes = A.state_dict_shapes(a)
    assert sorted(sd) == sorted(shapes)
    assert all(tuple(sd[k].shape) == tuple(shapes[k][0]) for k in sd)
    for k in ("backbone.stem.conv1.weight", "backbone.stem.conv1.norm.running_var", "backbone.res2.0.shortcut.weight",
              "backbone.res3.0.conv2.weight", "backbone.res5.2.conv3.norm.bias"):
        assert k in sd, k
    assert "backbone.res2.1.shortcut.weight" not in sd
    assert tuple(sd["backbone.res5.0.conv2.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["sem_seg_head.pixel_decoder.input_proj.0.0.weight"].shape) == (256, 2048, 1, 1)
    assert tuple(sd["sem_seg_head.pixel_decoder.adapter_1.weight"].shape) == (256, 256, 1, 1)


@pytest.mark.skipif(not os.path.isdir("/root/reference/configs"), reason="reference tree not present on this box")
def test_reference_resnet_and_densehybrid_configs_parse():
    """the reference's own R50 / R101 files (BASELINE config C1) and its DenseHybrid fine-tuning file resolve to our architectures"""
    from rba_amd.config import load_cfg
    base = "/root/reference/configs/cityscapes/semantic-segmentation/"
    a = A.arch_from_cfg(load_cfg(base + "maskformer2_R50_bs16_90k.yaml"))
    assert a["resnet"] == A.RESNET50 and a["dec_layers"] == 9 and a["enc_in"] == ["res3", "res4", "res5"]
    swin_only = ("object_mask_threshold", "overlap_threshold", "depths", "embed_dim", "num_heads", "window_size", "patch_size", "mlp_ratio")
    assert {k: v for k, v in a.items() if k not in swin_only} == \
        {k: v for k, v in A.complete(A.ARCHS["r50_9dl"]).items() if k not in swin_only}
    a = A.arch_from_cfg(load_cfg(base + "maskformer2_R101_bs16_90k_1dl.yaml"))
    assert a["resnet"]["depth"] == 101 and a["dec_layers"] == 1
    a = A.arch_from_cfg(load_cfg(base + "densehybrid/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_densehybrid_cocomix_finetune.yaml"))
    assert a["dense_hybrid"] is True and a["embed_dim"] == 128 and a["dec_layers"] == 1


def test_split_activations_layout_and_predicate():
    """ops.SplitActivations.pack is the layout contract of include/rba_hip.h ("Split activations"): checked element by element against
    the index formula, and unpack() inverts it; linear_takes_split mirrors the C dispatch (K > 256, >= 160 tiles, f16x3 mode)."""
    import numpy as np
    from rba_amd import ops
    g = torch.Generator().manual_seed(11)
    M, K = 70, 96
    x = torch.randn(M, K, generator=g) * 5
    sa = ops.SplitActivations.pack(x)
    assert sa.shape == (M, K) and sa.data.dtype == torch.int32 and sa.data.numel() == 96 * K      # rows padded to 96
    img = sa.data.view(torch.float16).numpy()
    h = x.half()
    l = ((x - h.float()) * 2048.0).half()
    NB = K // 32
    for row, k in ((0, 0), (1, 7), (31, 8), (32, 16), (33, 31), (69, 95), (45, 40), (64, 63)):
        rg, l31, b, half, gsel, i = row >> 5, row & 31, k >> 5, (k >> 4) & 1, (k >> 3) & 1, k & 7
        base = ((rg * NB + b) * 4096 + (2 * gsel) * 1024 + (half * 32 + l31) * 16) // 2 + i            # f16 units
        assert img[base] == h[row, k].numpy() and img[base + 512] == l[row, k].numpy()
    un = sa.unpack()
    assert un.shape == (M, K) and float((un - x).abs().max()) <= float(x.abs().max()) * 2.0 ** -21
    assert ops.SPLIT_MODE == "f16x3"
    if True:
        assert ops.linear_takes_split(8192, 2048, 512) and ops.linear_takes_split(8192, 512, 2048)
        assert ops.linear_takes_split(32768, 768, 256) and ops.linear_takes_split(131072, 384, 128)          # from K = 128 since round 3
        assert not ops.linear_takes_split(131072, 384, 96) and not ops.linear_takes_split(256, 1024, 1024)      # K below SPLIT_MIN_K / too few tiles
        assert ops.linear_takes_split(2048, 1024, 1024) and not ops.linear_takes_split(2048, 1024, 160)           # 128 tiles: the sub-tile kernel (K % 64, K >= 256)
        with ops.split_mode("bf16x6"):
            assert ops.SPLIT_MODE == "bf16x6" and not ops.linear_takes_split(8192, 2048, 512)
            import threading
            seen = []
            th = threading.Thread(target=lambda: seen.append(ops.SPLIT_MODE))           # round 5: the mode is per thread -- another thread keeps the default
            th.start(); th.join()
            assert seen == ["f16x3"]
        assert ops.SPLIT_MODE == "f16x3"
        with pytest.raises(AttributeError, match="split_mode"):                  # the pre-round-5 switch must fail loudly, not shadow the getter
            ops.SPLIT_MODE = "bf16x6"
        assert ops.SPLIT_MODE == "f16x3"


def test_shape_cache_pins_what_a_capture_reads(monkeypatch):
    """a hipGraph replay never calls ShapeCache.get, so entries a capture read must not be LRU victims."""
    from rba_amd import lru
    c = lru.ShapeCache(2)
    built = []

    def mk(k):
        return lambda: built.append(k) or ("v", k)
    c.get("a", mk("a"))
    c.get("b", mk("b"))
    monkeypatch.setattr(lru, "_capturing", lambda: True)
    assert c.get("a", mk("a")) == ("v", "a") and c.pinned() == 1           # read during a capture: pinned
    assert c.get("z", mk("z")) == ("v", "z") and "z" not in c._d and "z" not in c._pinned       # built during a capture: never shared
    monkeypatch.setattr(lru, "_capturing", lambda: False)
    for k in "cdefg":
        c.get(k, mk(k))
    assert c.get("a", mk("a")) == ("v", "a") and built.count("a") == 1    # survived five evictions
    assert len(c._d) == 2 and len(c) == 3
    c.get("b", mk("b"))
    assert built.count("b") == 2                                           # unpinned entries are still bounded


def test_heavy_recipe_and_seeded_labels(golden):
    """the trained-like stress recipe is deterministic, touches what it says, and the metric-parity fixtures' score-independent
    labels regenerate from their seeds"""
    from rba_amd.seeded_weights import seeded_ood_labels
    a = A.complete(A.ARCHS["swin_b_1dl"])
    base, heavy = A.seeded_weights(a, 0), A.seeded_weights(a, 0, recipe="heavy")
    assert all(torch.equal(heavy[k], v) for k, v in A.seeded_weights(a, 0, recipe="heavy").items())
    gam = heavy["backbone.layers.2.blocks.3.norm1.weight"]
    assert 0.1 <= gam.min() < 0.2 and 5 < gam.max() <= 10
    assert heavy["backbone.patch_embed.norm.bias"][77] < -600 and heavy["backbone.layers.2.blocks.0.mlp.fc2.bias"][5] > 900
    same = [k for k in base if torch.equal(base[k], heavy[k])]
    assert "backbone.layers.0.blocks.0.attn.qkv.weight" in same and "backbone.layers.2.blocks.3.norm1.weight" not in same
    for fixture in ("g7_metrics_swin_b_9dl_720x1280", "g7_metrics_swin_b_1dl_1024x2048"):
        g = golden(fixture)
        h, w = (int(v) for v in g["hw"])
        off = int(g["label_seed_offsets"][0])
        labs = [seeded_ood_labels(h, w, off + int(s)) for s in g["img_seeds"]]
        assert sum(int((l == 1).sum()) for l in labs) == int(g["n_ood"][0])
        assert all(int((l == 255).sum()) == h * w - (h - 32) * (w - 32) for l in labs)
        bits = np.unpackbits(g["labels_corr_bits"], axis=1)[:, : h * w]
        assert int(bits.sum()) == int(g["n_ood"][1])
        assert 0.80 < float(g["metrics_corr"][0]) < 0.85 and abs(float(g["metrics_indep"][0]) - 0.5) < 0.01


def test_checkpoint_pickle_with_torch_tensors_is_refused_with_a_hint(tmp_path):
    """tools/convert-pretrained-swin-model-to-d2.py pickles torch tensors: refused by default, the message says how to opt in"""
    from rba_amd.checkpoint import read_state_dict
    pth = tmp_path / "swin.pkl"
    with open(pth, "wb") as f:
        pickle.dump({"model": {"w": torch.ones(2, 2)}, "matching_heuristics": True}, f)
    with pytest.raises(pickle.UnpicklingError, match="RBA_TRUSTED_CHECKPOINT=1"):
        read_state_dict(str(pth))
    assert torch.equal(read_state_dict(str(pth), trusted=True)["w"], torch.ones(2, 2))


def test_to_device_is_a_plain_move_without_a_hip_device():
    from rba_amd.h2d import to_device
    x = torch.arange(6).view(2, 3)
    assert to_device(x, "cpu") is x or torch.equal(to_device(x, "cpu"), x)
    assert to_device(None, "cpu") is None


def test_emitted_isa_has_no_unfenced_16bit_destination_hazards():
    """hipcc separates a 16-bit-destination VALU (v_fma_mixlo/mixhi_f16 ...) and a transcendental from the next VALU that reads the register
    when it emitted both; it cannot look inside `asm`.  Scan EVERY gfx950 code object of the built library for back-to-back pairs
    (tools/isa_hazards.py): round 3's fused K1 (rba_reduce_up4_mx_kernel) shipped with 40 of them (measured harmless on MI355X,
    profiles/r04_mix_hazard_probe.txt -- but the rule is the compiler's own, so the library is kept clean of them)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_hazards
    from rba_amd import _lib
    if not os.path.exists(os.path.join(isa_hazards.LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    r = isa_hazards.scan_library(_lib.LIB_PATH)
    assert r["code_objects"] >= 15 and r["mix"] > 3000, r["code_objects"]      # the scan saw the library's kernels (3 452 v_fma_mix* in round 4)
    assert not r["D"], r["D"][:3]
    assert not r["T"], r["T"][:3]
    # round 5: no packed fp32 instruction with the cross select on source 1 (`op_sel:[x,1]`): the form that produced zero products in the GroupNorm fold
    # (csrc/split_linear_gnf.hip, profiles/r05_gnfold_select.txt)
    assert not r["P"], r["P"][:3]
    # the scanner itself: the round-3 pattern must be flagged, the fenced forms must pass
    mk = lambda *ins: [("label", "k")] + [(i, "k") for i in ins]
    lo, hi = "v_fma_mixlo_f16 v24, v20, v9, v11 op_sel_hi:[1,0,0]", "v_fma_mixhi_f16 v24, v20, v9, v14 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
    assert len(isa_hazards.scan(mk(lo, hi))["D"]) == 1
    assert not isa_hazards.scan(mk(lo, "s_nop 0", hi))["D"]
    assert not isa_hazards.scan(mk(lo, lo.replace("v24", "v25"), hi))["D"]
    assert len(isa_hazards.scan(mk(hi, "v_mfma_f32_32x32x16_f16 v[0:15], v[16:19], v[24:27], v[0:15]"))["D"]) == 1
    assert not isa_hazards.scan(mk(hi, "ds_write_b128 v2, v[24:27]"))["D"]        # not a VALU reader
    assert len(isa_hazards.scan(mk("v_rcp_f32_e32 v4, v1", "v_mul_f32_e32 v5, v4, v4"))["T"]) == 1
    assert not isa_hazards.scan(mk("v_rcp_f32_e32 v4, v1", "v_exp_f32_e32 v5, v4"))["T"]
    assert len(isa_hazards.scan(mk("v_pk_mul_f32 v[166:167], v[130:131], v[182:183] op_sel:[0,1]"))["P"]) == 1
    assert len(isa_hazards.scan(mk("v_pk_add_f32 v[68:69], v[68:69], v[68:69] op_sel:[0,1] op_sel_hi:[1,0]"))["P"]) == 1
    assert not isa_hazards.scan(mk("v_pk_mul_f32 v[166:167], v[182:183], v[130:131] op_sel:[1,0]", "v_pk_mul_f32 v[2:3], v[4:5], v[6:7] op_sel_hi:[0,1]",
                                   "v_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel:[0,0,1] op_sel_hi:[1,1,0]"))["P"]


def test_build_gates_both_libraries_on_the_isa_scan(tmp_path):
    """correctness must not depend on this test file.  rba_amd/csrc/build.py links to `<lib>.unscanned`, runs
    isa_hazards.gate on it and only then renames it -- for the product library AND the knobs build.  Checked here: (1) the knobs library on disk is clean
    too; (2) gate() raises on a code object that holds the rule-P form (the erratum reproducer tools/micro/pk_opsel_after_load.hip, compiled here) and the
    build's link step then leaves no library behind."""
    import subprocess
    from rba_amd import _lib
    from rba_amd.csrc import build as B, isa_hazards
    if not os.path.exists(os.path.join(isa_hazards.LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    if os.path.exists(_lib.KNOBS_LIB_PATH):
        r = isa_hazards.gate(_lib.KNOBS_LIB_PATH)
        assert r["code_objects"] >= 15
    obj = str(tmp_path / "pk.o")
    subprocess.run([B.HIPCC] + B.FLAGS + ["-c", os.path.join(REPO, "tools", "micro", "pk_opsel_after_load.hip"), "-o", obj], check=True,
                   stderr=subprocess.DEVNULL)
    assert isa_hazards.scan_library(obj)["P"], "the reproducer no longer contains the form: the gate would be untested"
    with pytest.raises(RuntimeError, match="cross select on source 1"):
        isa_hazards.gate(obj)
    lib = str(tmp_path / "libbad.so")
    with pytest.raises(RuntimeError):
        B._link_and_gate([obj], lib, verbose=False)
    assert not os.path.exists(lib) and not os.path.exists(lib + ".unscanned")
    good = os.path.join(B.OBJ, "layer_norm.o")
    if os.path.exists(good):
        B._link_and_gate([good], lib, verbose=False)
        assert os.path.exists(lib) and not os.path.exists(lib + ".unscanned")


def test_bench_names_its_workload_and_configs2_flag():
    """VERDICT r3 #5d: `--gpus 8 --images-per-gpu 2` is exactly BASELINE configs[2] (batch 16 sharded 8x) and the line says so; any other shape of the
    run is labelled as what it is.  The flag is an alias of --streams (one image per stream per step)."""
    import bench
    assert "configs[2]: batch 16" in bench.baseline_config("swin_b_1dl", 1024, 2048, 8, 2)
    assert "configs[1]" in bench.baseline_config("swin_b_1dl", 1024, 2048, 1, 3) and "configs[2] exactly = --gpus 8 --images-per-gpu 2" in bench.baseline_config("swin_b_1dl", 1024, 2048, 8, 3)
    assert bench.baseline_config("swin_l_1dl", 1024, 2048) == "BASELINE.json configs[3]" and bench.baseline_config("swin_b_9dl", 720, 1280) == "BASELINE.json configs[4]"
    assert bench.baseline_config("swin_b_1dl", 512, 512) == "not a BASELINE.json configuration"
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8", "--images-per-gpu", "2"]
        a = bench.parse()
        assert a.streams == 2 and a.gpus == 8 and a.graph == 1 and a.cpu_baseline == "quick" and a.sustain == 5.0
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert a.streams == 3 and a.gpus == 1 and a.steps == 20 and a.warmup == 3
        assert a.full is False and a.dump_outputs is None                   # a plain run: headline only, nothing written
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out", "--steps", "7"]
        a = bench.parse()
        assert a.full is True and a.dump_outputs == "out" and a.steps == 7
    finally:
        sys.argv = old


def test_bench_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    """bench.dump_outputs: the maps of one step stacked as float32 [n, H, W] in rba.npy; above the size limit, the same strided sub-grid of every map."""
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(3)
    maps = [torch.randn(40, 70, generator=g) for _ in range(3)]
    bench.dump_outputs(str(tmp_path / "a"), maps)
    got = np.load(tmp_path / "a" / "rba.npy")
    assert got.dtype == np.float32 and got.shape == (3, 40, 70) and np.array_equal(got, torch.stack(maps).numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 20 * 35 * 4)
    bench.dump_outputs(str(tmp_path / "b"), maps)
    got = np.load(tmp_path / "b" / "rba.npy")
    assert got.nbytes <= bench.DUMP_LIMIT_BYTES and np.array_equal(got, torch.stack(maps).numpy()[:, ::2, ::2])


def test_registries_hold_the_reference_names():
    """the names a reference config.yaml selects components by (META_ARCHITECTURE, BACKBONE.NAME, SEM_SEG_HEAD.NAME, PIXEL_DECODER_NAME,
    TRANSFORMER_DECODER_NAME) resolve in the registries -- a decorator separated from its class shows up here, not on the GPU box"""
    import rba_amd.maskformer_model  # noqa: F401  (imports register everything)
    from rba_amd import registry as R
    for reg, names in ((R.META_ARCH_REGISTRY, ["MaskFormer"]), (R.BACKBONE_REGISTRY, ["D2SwinTransformer", "build_resnet_backbone"]),
                       (R.SEM_SEG_HEADS_REGISTRY, ["MaskFormerHead", "MSDeformAttnPixelDecoder"]),
                       (R.TRANSFORMER_DECODER_REGISTRY, ["MultiScaleMaskedTransformerDecoder"])):
        for n in names:
            assert isinstance(reg.get(n), type) or callable(reg.get(n)), n


def _write_d2_checkpoints(folder, sd):
    """the three on-disk forms a released / converted checkpoint comes in: Detectron2's periodic checkpointer (`model_final.pth`: model + optimizer + scheduler +
    iteration, detectron2/checkpoint via fvcore Checkpointer.save), the model-zoo `.pkl` (numpy arrays, `__author__`, `matching_heuristics`), and the `.pkl` the
    reference's own converter writes -- torch tensors inside a plain pickle (tools/convert-pretrained-swin-model-to-d2.py:22-30)"""
    import pickle
    os.makedirs(folder, exist_ok=True)
    opt = {"state": {0: {"step": torch.tensor(90000.0), "exp_avg": torch.zeros(3)}}, "param_groups": [{"lr": 1e-4, "params": [0]}]}
    torch.save({"model": dict(sd, **{"criterion.empty_weight": torch.ones(20)}), "optimizer": opt, "scheduler": {"last_epoch": 90000, "_step_count": 90001},
                "iteration": 89999}, os.path.join(folder, "model_final.pth"))
    with open(os.path.join(folder, "numpy.pkl"), "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "third_party", "matching_heuristics": True}, f)
    with open(os.path.join(folder, "tensors.pkl"), "wb") as f:
        pickle.dump({"model": dict(sd), "__author__": "third_party", "matching_heuristics": True}, f)


def test_model_zoo_check_table_checkpoint_formats_and_comparison(tmp_path, capsys):
    """tools/model_zoo_check.py (SURVEY 8(f) f1 made turnkey): (1) its table IS the reference's MODEL_ZOO.md (parsed here when the reference tree is present);
    (2) the checkpoint files exactly as Detectron2 and the reference's converter write them load into the model on the CPU, key for key; (3) the comparison:
    published vs results.pkl in percentage points, exit status, missing entries, --dry-run -- everything except the GPU run itself (tests/test_model_gpu.py)."""
    import pickle
    import re
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import model_zoo_check as Z
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint, read_state_dict
    from rba_amd.maskformer_model import MaskFormer
    # (1) the table
    zoo = "/root/reference/MODEL_ZOO.md"
    if os.path.exists(zoo):
        txt = open(zoo).read()
        rows = re.findall(r'<tr><td align="left">.*?</tr>', txt, flags=re.S)
        got = {}
        for r in rows:
            cfg = re.search(r'ckpts/([a-z0-9_]+)/config.yaml', r).group(1)
            nums = [float(x) for x in re.findall(r'<td align="center">([0-9.]+)</td>', r)]
            got[cfg] = nums[-4:]                                   # ..., RA AP, RA FPR95, FS-LaF AP, FS-LaF FPR95
        assert sorted(got) == sorted(Z.MODEL_ZOO)
        for m, (ra_ap, ra_fpr, fs_ap, fs_fpr) in got.items():
            t = Z.MODEL_ZOO[m]
            assert (t["road_anomaly"]["aupr"], t["road_anomaly"]["fpr95"], t["fishyscapes_laf"]["aupr"], t["fishyscapes_laf"]["fpr95"]) == (ra_ap, ra_fpr, fs_ap, fs_fpr), m
    assert Z.MODEL_ZOO["swin_b_1dl"]["road_anomaly"] == {"aupr": 78.45, "fpr95": 11.83}          # BASELINE.json's target row
    # (2) checkpoint formats
    a = A.complete(A.ARCHS["tiny1"])
    sd = A.seeded_weights(a, 0)
    ck = tmp_path / "ck"
    _write_d2_checkpoints(str(ck), sd)
    want = load_checkpoint(MaskFormer(a), sd).state_dict()
    for fname, trusted in (("model_final.pth", False), ("numpy.pkl", False), ("tensors.pkl", True)):
        got_sd = load_checkpoint(MaskFormer(a), str(ck / fname), trusted=trusted).state_dict()
        assert sorted(got_sd) == sorted(want) and all(torch.equal(got_sd[k], want[k]) for k in want), fname
    with pytest.raises(pickle.UnpicklingError, match="RBA_TRUSTED_CHECKPOINT"):
        read_state_dict(str(ck / "tensors.pkl"))                                               # torch tensors in a pickle: refused unless trusted
    # (3) the comparison
    models = tmp_path / "ckpts"
    for m in ("swin_b_1dl", "swin_l_1dl", "not_in_the_table"):
        (models / m).mkdir(parents=True)
        (models / m / "config.yaml").write_text("MODEL: {}\n")
    (models / "swin_b_1dl" / "model_final.pth").write_bytes(b"")
    out = tmp_path / "results"
    (out / "swin_b_1dl").mkdir(parents=True)
    exact = {ds: {k: v / 100.0 for k, v in Z.MODEL_ZOO["swin_b_1dl"][ds].items()} for ds in Z.DATASETS}
    exact["road_anomaly"]["auroc"] = 0.97
    with open(out / "swin_b_1dl" / "results.pkl", "wb") as f:
        pickle.dump(exact, f)
    base = ["--models_folder", str(models), "--datasets_folder", str(tmp_path), "--out_path", str(out), "--selected_models", "swin_b_1dl"]
    assert Z.main(base + ["--dry-run"]) == 0
    assert "swin_b_1dl: config.yaml found, checkpoint" in capsys.readouterr().out
    assert Z.main(base + ["--results-only"]) == 0
    txt = capsys.readouterr().out
    assert "4 of 4 published numbers reproduced" in txt and "78.45" in txt
    exact["road_anomaly"]["aupr"] += 0.0004                                                    # 0.04 percentage points: outside 0.005, inside "three decimals"
    with open(out / "swin_b_1dl" / "results.pkl", "wb") as f:
        pickle.dump(exact, f)
    assert Z.main(base + ["--results-only"]) == 1
    assert "DIFFERS" in capsys.readouterr().out
    assert Z.main(base + ["--results-only", "--tolerance", "0.05"]) == 0
    capsys.readouterr()
    assert Z.main(["--models_folder", str(models), "--out_path", str(out), "--results-only"]) == 1          # swin_l_1dl has no results.pkl: MISSING rows
    assert "MISSING" in capsys.readouterr().out
    assert Z.main(["--models_folder", str(models), "--out_path", str(out), "--selected_models", "not_in_the_table", "--results-only"]) == 2


def _cpu_model(name, seed=0):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[name])
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, seed)).eval(), a


def _replace_param(mod, attr, like=None):
    """`mod.<attr> = nn.Parameter(new values)`; returns the old Parameter"""
    old = getattr(mod, attr)
    new = (old.detach() * 1.25 + 0.01) if like is None else like
    setattr(mod, attr, torch.nn.Parameter(new.clone()))
    return old


def _set_data(p):
    p.data = p.detach() * 0.75 - 0.02


@torch.no_grad()
def _in_place(t):
    t.mul_(1.0)                                   # same values, new version: an in-place edit as load_state_dict / an optimiser step makes it


@pytest.mark.parametrize("name", ["tiny1", "r50_1dl"])
def test_weights_key_follows_every_kind_of_weight_change(name):
    """The weights' part of MaskFormer's graph key changes under every way of changing a weight -- load_state_dict (copy and assign=True), a submodule swap,
    a new Parameter set on a module, `p.data = t`, in-place edits of a parameter and of a buffer -- is stable while nothing changes, walks the module tree
    only after a registration (never per call), and lets go of replaced Parameters."""
    import gc
    import weakref
    from rba_amd.maskformer_model import MaskFormer
    model, a = _cpu_model(name)
    sd1 = A.seeded_weights(a, 1)
    mods = dict(model.named_modules())
    pred = model.sem_seg_head.predictor
    conv_bn = model.backbone.stem.conv1 if name == "r50_1dl" else None
    params = ["sem_seg_head.predictor.query_feat.weight", "sem_seg_head.predictor.decoder_norm.weight",
              "sem_seg_head.predictor.transformer_cross_attention_layers.0.multihead_attn.in_proj_weight",
              "sem_seg_head.pixel_decoder.transformer.encoder.layers.0.self_attn.value_proj.weight"]
    if name == "tiny1":
        params += ["backbone.layers.0.blocks.0.mlp.fc1.weight", "backbone.layers.0.blocks.0.attn.qkv.weight",
                   "backbone.layers.0.blocks.0.attn.relative_position_bias_table"]
    else:
        params += ["backbone.stem.conv1.weight", "backbone.res2.0.conv1.norm.bias"]

    def owner(path):
        m_, _, attr = path.rpartition(".")
        return mods[m_] if m_ else model, attr

    changes = [("load_state_dict copy", lambda: model.load_state_dict(sd1, strict=False)),
               ("load_state_dict assign", lambda: model.load_state_dict({k: v.clone() for k, v in sd1.items()}, strict=False, assign=True)),
               ("class_embed swap", lambda: setattr(pred, "class_embed", torch.nn.Linear(pred.class_embed.in_features, pred.class_embed.out_features)))]
    for path in params:
        changes.append((f"new Parameter {path}", lambda path=path: _replace_param(*owner(path))))
        changes.append((f".data = {path}", lambda path=path: _set_data(getattr(*owner(path)))))
        changes.append((f"in-place {path}", lambda path=path: _in_place(getattr(*owner(path)))))
    if conv_bn is not None:
        changes.append(("in-place running_mean", lambda: conv_bn.norm.running_mean.add_(0.5)))
        changes.append(("in-place running_var", lambda: conv_bn.norm.running_var.mul_(2.0)))
        changes.append(("new running_mean buffer", lambda: setattr(conv_bn.norm, "running_mean", conv_bn.norm.running_mean + 1.0)))
    else:
        idx = mods["backbone.layers.0.blocks.0.attn"].relative_position_index
        changes.append(("in-place relative_position_index", lambda: idx.add_(0)))
    changes.append(("in-place pixel_mean buffer", lambda: model.pixel_mean.add_(0.0)))
    v = model._weights_version()
    assert model._weights_version() == v
    for what, change in changes:
        change()
        v1 = model._weights_version()
        assert v1 != v, what
        assert model._weights_version() == v1, what                     # stable while nothing changes
        v = v1

    # no module walk per call: after the first call the flat list serves every call until something is registered
    flat_parameters, flat_buffers = MaskFormer.parameters, MaskFormer.buffers

    def walked(*args, **kwargs):
        raise AssertionError("_weights_version walked the module tree on a call where nothing was registered")
    try:
        MaskFormer.parameters, MaskFormer.buffers = walked, walked
        for _ in range(3):
            assert model._weights_version() == v
    finally:
        MaskFormer.parameters, MaskFormer.buffers = flat_parameters, flat_buffers

    # replaced Parameters are not kept alive by the key's flat list
    w_old = weakref.ref(pred.decoder_norm.weight)
    b_old = weakref.ref(_replace_param(pred.class_embed, "bias"))
    pred.decoder_norm.weight = torch.nn.Parameter(pred.decoder_norm.weight.detach() + 1.0)
    assert model._weights_version() != v
    gc.collect()
    assert w_old() is None and b_old() is None


def _edits(mod, attr, buffer=False, positive=False):
    """the ways a source tensor changes: in place, `.data =` (parameters), replaced by a new Parameter / buffer tensor"""
    def val(t):
        return (t.detach() * 1.5 + 0.25).abs() + 0.5 if positive else t.detach() * 1.5 - 0.25

    @torch.no_grad()
    def in_place():
        t = getattr(mod, attr)
        t.copy_(val(t))

    def set_data():
        t = getattr(mod, attr)
        t.data = val(t).clone()

    def replace():
        t = val(getattr(mod, attr)).clone()
        setattr(mod, attr, t if buffer else torch.nn.Parameter(t))
    return [(f"{attr} in place", in_place), (f"{attr} replaced", replace)] + ([] if buffer else [(f"{attr}.data =", set_data)])


def test_conv_bn_fold_follows_all_five_sources():
    """ResNet's ConvBN.folded() (BatchNorm folded into the convolution, cached per weight load) is rebuilt when ANY of weight, norm.weight, norm.bias,
    norm.running_mean, norm.running_var changes -- in place or by replacement -- and equals a fresh fold and a float64 fold to fp32 rounding."""
    from rba_amd.modeling.backbone.resnet import ConvBN
    torch.manual_seed(0)
    cb = ConvBN(8, 16, 3, padding=1).eval()
    with torch.no_grad():
        cb.norm.weight.uniform_(0.5, 1.5); cb.norm.bias.uniform_(-1, 1)
        cb.norm.running_mean.uniform_(-1, 1); cb.norm.running_var.uniform_(0.5, 2.0)
    edits = (_edits(cb, "weight") + _edits(cb.norm, "weight") + _edits(cb.norm, "bias")
             + _edits(cb.norm, "running_mean", buffer=True) + _edits(cb.norm, "running_var", buffer=True, positive=True))
    for what, edit in [("initial", lambda: None)] + edits:
        before = [t.clone() for t in cb.folded()]
        edit()
        w, b = cb.folded()
        fresh = ConvBN(8, 16, 3, padding=1).eval()
        fresh.load_state_dict(cb.state_dict())
        fw, fb = fresh.folded()
        assert torch.equal(w, fw) and torch.equal(b, fb), what
        if what != "initial":
            assert not (torch.equal(w, before[0]) and torch.equal(b, before[1])), what
        n = cb.norm
        scale = n.weight.double() / torch.sqrt(n.running_var.double() + n.eps)
        w64 = cb.weight.double() * scale.view(-1, 1, 1, 1)
        b64 = n.bias.double() - n.running_mean.double() * scale
        eps32 = 2.0 ** -23
        assert ((w.double() - w64).abs() <= 4 * eps32 * w64.abs() + 1e-30).all(), what
        assert ((b.double() - b64).abs() <= 4 * eps32 * (n.bias.double().abs() + (n.running_mean.double() * scale).abs())).all(), what


def test_weight_derived_views_follow_every_source():
    """The weight-derived caches that are built on the host -- Swin's gathered relative-position bias, the decoder's key / value views of in_proj, the
    PatchEmbed projection as a Linear view, the stacked sampling Linear of MSDeformAttn and the pixel decoder's 1x1-convolution views -- are rebuilt when any
    of their sources is edited in place or replaced, and equal a fresh derivation."""
    from rba_amd.modeling.pixel_decoder.msdeformattn import _cached_linear_view
    model, a = _cpu_model("tiny1")
    mods = dict(model.named_modules())
    attn = mods["backbone.layers.0.blocks.1.attn"]
    N = attn.window_size ** 2

    def check_bias():
        b, frag = attn.gathered_bias()
        t, idx = attn.relative_position_bias_table, attn.relative_position_index
        return frag is None and torch.equal(b, t[idx.view(-1)].view(N, N, -1).permute(2, 0, 1))

    mha = mods["sem_seg_head.predictor.transformer_cross_attention_layers.0.multihead_attn"]
    E = mha.embed_dim

    def check_kv():
        lk, lv = mha._kv_views()
        w, b = mha.in_proj_weight, mha.in_proj_bias
        return (torch.equal(lk.weight, w[E:2 * E]) and torch.equal(lk.bias, b[E:2 * E]) and torch.equal(lv.weight, w[2 * E:])
                and torch.equal(lv.bias, b[2 * E:]))

    pe = model.backbone.patch_embed

    def check_pe():
        v = pe._linear_view()
        return torch.equal(v.weight, pe.proj.weight.reshape(pe.proj.weight.shape[0], -1)) and torch.equal(v.bias, pe.proj.bias)

    msda = mods["sem_seg_head.pixel_decoder.transformer.encoder.layers.0.self_attn"]

    def check_sampling():
        lin = msda._sampling_linear()
        so, aw = msda.sampling_offsets, msda.attention_weights
        return torch.equal(lin.weight, torch.cat([so.weight, aw.weight])) and torch.equal(lin.bias, torch.cat([so.bias, aw.bias]))

    conv = model.sem_seg_head.pixel_decoder.mask_features

    def check_conv_view():
        v = _cached_linear_view(conv)
        return torch.equal(v.weight, conv.weight.view(conv.weight.shape[0], -1)) and torch.equal(v.bias, conv.bias)

    cases = [(check_bias, _edits(attn, "relative_position_bias_table")
              + [("index in place", lambda: attn.relative_position_index.copy_(attn.relative_position_index.flip(0).clone())),
                 ("index replaced", lambda: setattr(attn, "relative_position_index", attn.relative_position_index.flip(1).clone()))]),
             (check_kv, _edits(mha, "in_proj_weight") + _edits(mha, "in_proj_bias")),
             (check_pe, _edits(pe.proj, "weight") + _edits(pe.proj, "bias")),
             (check_sampling, _edits(msda.sampling_offsets, "weight") + _edits(msda.sampling_offsets, "bias")
              + _edits(msda.attention_weights, "weight") + _edits(msda.attention_weights, "bias")),
             (check_conv_view, _edits(conv, "weight") + _edits(conv, "bias"))]
    with torch.no_grad():
        for check, edits in cases:
            assert check(), check.__name__
            for what, edit in edits:
                edit()
                assert check(), (check.__name__, what)
