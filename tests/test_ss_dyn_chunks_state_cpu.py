"""CPU: what tests/test_gpu_ss_dyn_chunks_state.py trusts, pinned before anything on the GPU uses it -- the row-level fp64
recursion of tests/ss_rows_ref.py against the fp64 tree of tests/asym_pot_tree_ref.py on the circuit's own rows (float64, from
its probe tape), a split run carried through zT -> z0, the committed seeds of the cases with more than one state in chunks, and
the chunk geometry those cases are cut in."""
import numpy as np
import pytest

import ss_dyn_asym_cases as cases
import ss_rows_ref as rref

NEW_CASES = ["two_state_vs2_c", "three_state_c", "three_state_r1", "four_state_c", "four_state_vs", "four_state_vs_seq"]


@pytest.fixture(scope="module")
def rows_case(oracle):
    """name -> (circ, rows float64, x [B,T,ni] float64, the exact two-diode root, y of the fp64 tree); once per case."""
    import tf_wdf as W
    memo = {}

    def get(name):
        if name not in memo:
            x, _, r = cases.data(name)
            circ, _ = cases.build(W, name)
            x64 = x.astype(np.float64).reshape(x.shape[0], x.shape[1], -1)
            f, theta = cases.forward_of(oracle, name, x.astype(np.float64), r)
            memo[name] = (circ, rref.rows_of(circ, r), x64, rref.root_asym(oracle, theta[-4:]), f(theta))
        return memo[name]
    return get


@pytest.mark.parametrize("name", ["two_state_vs2_c", "four_state_vs"])
def test_rows_recursion_on_the_circuits_own_rows_is_the_tree(rows_case, name):
    """The rows of the probe tape in float64 (a row per sample: the pot moves), run through the recursion the kernel header
    states, against the tree that propagates its impedances again at every step: the same circuit, two formulations."""
    circ, rows, x64, root, y_tree = rows_case(name)
    B, T, ni = cases.CASES[name]["shape"]
    assert (circ.ns, circ.ni) == ({"two_state": 2, "four_state": 4}[cases.CASES[name]["tree"]], ni)
    assert rows.shape == (T, rref.row_len(circ.ns, ni), B)
    y, zT = rref.run(rows, x64, circ.ns, ni, root)
    d = float(np.max(np.abs(y - y_tree)))
    print(f"{name}: rows recursion against the tree: max |dy| = {d:.3g} V")
    assert y.shape == (T, B) and zT.shape == (circ.ns, B) and d <= 1e-9


@pytest.mark.parametrize("name", ["two_state_vs2_c", "four_state_vs"])
def test_rows_recursion_split_and_carried_equals_the_unsplit_run(rows_case, name):
    circ, rows, x64, root, _ = rows_case(name)
    ns, ni, T = circ.ns, circ.ni, x64.shape[1]
    y, zT = rref.run(rows, x64, ns, ni, root)
    y1, z1 = rref.run(rref.time_slice(rows, 0, 57), x64[:, :57], ns, ni, root)
    y2, z2 = rref.run(rref.time_slice(rows, 57, T), x64[:, 57:], ns, ni, root, z0=z1)
    dy, dz = float(np.max(np.abs(np.concatenate([y1, y2]) - y))), float(np.max(np.abs(z2 - zT)))
    print(f"{name}: split at 57: max |dy| = {dy:.3g}, max |dzT| = {dz:.3g}")
    assert dy <= 1e-12 and dz <= 1e-12
    assert float(np.max(np.abs(z1))) > 1e-3                               # (the carried state is not a zero that proves nothing)


def test_rows_recursion_layouts_and_gz0():
    """One static row [n], the same row per sequence [1,n,B] and per sample [T,n,B] give the same bits; on a linear tree (no root)
    dL/dz0 by differences is the closed form sum_t gy_t cy A^t."""
    rng = np.random.default_rng(0)
    ns, ni, B, T = 2, 2, 3, 9
    n = rref.row_len(ns, ni)
    row = rng.uniform(-0.4, 0.4, n)
    x, z0, gy = rng.standard_normal((B, T, ni)), rng.uniform(-0.2, 0.2, (ns, B)), rng.standard_normal((T, B))
    y, zT = rref.run(row, x, ns, ni, z0=z0)
    for rows in (np.repeat(row[None, :, None], B, axis=2), np.broadcast_to(row[None, :, None], (T, n, B))):
        y2, zT2 = rref.run(rows, x, ns, ni, z0=z0)
        assert np.array_equal(y2, y) and np.array_equal(zT2, zT)
    A, cy = row[:ns * ns].reshape(ns, ns), row[ns * ns + ns * ni + 2 * ns + ni:][:ns]
    want, v = np.zeros((ns, B)), cy.copy()
    for t in range(T):
        want += v[:, None] * gy[t][None, :]
        v = v @ A
    got = rref.grad_z0(row, x, ns, ni, rref.root_none, z0, gy)
    assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))


@pytest.mark.parametrize("name", NEW_CASES)
def test_new_cases_commit_the_first_balanced_seed(oracle, name):
    seed = cases.CASES[name]["seed"]
    assert cases.find_seed(oracle, name) == seed
    bal = cases.reference(oracle, name)["balance"]
    print(f"{name}: seed {seed}, smallest balance {bal.min():.3g}")
    assert np.all(bal >= cases.BALANCE) and cases.BALANCE == 0.03


def test_chunk_geometry_of_the_new_cases():
    """131 steps in four chunks of 8-step units: 40, 40, 40 and 11 -- the last chunk ragged and no whole unit; asked for 16 chunks
    the library cuts 9 of 16 steps (the last: 3), asked for 17 it cuts 17 of 8 (the last: 3)."""
    from wdf_hip import binding
    assert binding.chunk_geom(131, 4, 8) == (40, 4)
    assert binding.chunk_geom(131, 16, 8) == (16, 9) and binding.dyn_chunks(131, 16) == 9
    assert binding.chunk_geom(131, 17, 8) == (8, 17) and binding.dyn_chunks(131, 17) == 17
    for name in NEW_CASES:
        assert cases.CASES[name]["shape"][:2] == (70, 131)
