"""CompiledCircuit::solve_witness of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) on the README circuit."""
import pytest

from test_host_mirror import _run


@pytest.mark.gpu
def test_solve_witness_through_the_cpp_mirror(built):
    out = _run("test_witness_solve_host")
    for t in ("honest ok", "wrong input ok", "refusals ok"):
        assert t in out
