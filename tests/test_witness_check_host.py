"""CompiledCircuit::check_witness of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) on the README circuit."""
import pytest

from test_host_mirror import _run


@pytest.mark.gpu
def test_check_witness_through_the_cpp_mirror(built):
    out = _run("test_witness_check_host")
    for t in ("honest ok", "wrong input ok", "corrupted cell ok"):
        assert t in out
