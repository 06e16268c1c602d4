"""Child process of test_ragged_dropout_gpu.py::test_fma_ragged_attention_backward_draws_the_same_masks: the named cases of
tests/ragged_cases.py through one skip-padding training step with dropout under STLT_ATTN_BWD16=0 (the library reads its switches once per
process, so the parent puts it in the environment); exits non-zero unless each case is within the GPU test's bounds of the ragged oracle
AND the launch recorder shows both towers' attention backward on the plain-FMA attn_bwd_kernel (the switch took effect)."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from conftest import PKG_NAME  # noqa: E402
from ragged_cases import assert_routes, build_model, check_step, logit_bound, ragged_reference, train_step  # noqa: E402


def main():
    assert os.environ.get("STLT_ATTN_BWD16") == "0"
    pkg = importlib.import_module(PKG_NAME)
    for name in sys.argv[1:]:
        m = build_model(pkg, name)
        check_step(f"{name} ragged, STLT_ATTN_BWD16=0", name, train_step(m, name, True), ragged_reference(name), logit_bound(name))
        assert_routes(pkg, m, name, sp=("fma", 0), tp=("fma", 0))


if __name__ == "__main__":
    main()
