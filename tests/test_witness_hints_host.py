"""CompiledCircuit::set_hints of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) on the README circuit."""
import pytest

from test_host_mirror import _run


@pytest.mark.gpu
def test_set_hints_through_the_cpp_mirror(built):
    out = _run("test_witness_hints_host")
    for t in ("hinted ok", "refusals ok", "removed ok"):
        assert t in out
