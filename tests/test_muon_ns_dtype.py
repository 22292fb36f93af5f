"""Build-only config key ``muon_ns_dtype`` (optim/factory.py) -> Muon(ns_dtype=...): the Newton-Schulz
arithmetic, "bfloat16" (default) or "float32" (csrc/muon_ns_f32.hip).  No GPU needed: only the factory
and the constructor run."""
import pytest


def test_factory_passes_muon_ns_dtype_through():
    from plaincv_amd.optim.factory import get_optimizer
    from utils import Config
    assert get_optimizer(Config(optim="muon", lr=1e-3)).ns_dtype == "bfloat16"
    assert get_optimizer(Config(optim="muon", lr=1e-3, muon_ns_dtype="bfloat16")).ns_dtype == "bfloat16"
    assert get_optimizer(Config(optim="muon", lr=1e-3, muon_ns_dtype="float32")).ns_dtype == "float32"
    assert get_optimizer({"optim": "muon", "muon_ns_dtype": "float32"}).ns_dtype == "float32"
    sf = get_optimizer(Config(optim="muon", lr=1e-3, muon_ns_dtype="float32", schedule_free=True))
    assert sf.base.ns_dtype == "float32"


def test_muon_ns_dtype_default_and_validation():
    from plaincv_amd.optim.factory import get_optimizer
    from plaincv_amd.optim.muon import Muon
    from utils import Config
    assert Muon(1e-3).ns_dtype == "bfloat16"
    assert Muon(1e-3, ns_dtype="float32").ns_dtype == "float32"
    for bad in ("float16", "fp32", "", "Float32", None):
        with pytest.raises(ValueError):
            Muon(1e-3, ns_dtype=bad)
    with pytest.raises(ValueError):
        get_optimizer(Config(optim="muon", lr=1e-3, muon_ns_dtype="float64"))


def test_other_optimizers_ignore_muon_ns_dtype():
    from plaincv_amd.optim.factory import get_optimizer
    from utils import Config
    for name in ("adamw", "soap", "shampoo", "signum"):
        get_optimizer(Config(optim=name, lr=1e-3, muon_ns_dtype="float32"))
