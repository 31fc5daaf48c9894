"""CPU tier: every built library holds exactly the kernels tests/kernel_inventory.py lists -- each kernel under exactly one key, each
key's count exact, nothing left over -- and the `static` scan kernels, which every code object that includes them would carry under
the same name, are in msm.hip's objects only."""
import pytest

import kernel_inventory as inv


@pytest.mark.parametrize("libname", sorted(inv.INVENTORY))
def test_library_holds_its_inventory(libname):
    table, names = inv.INVENTORY[libname], sorted(inv.kernels(libname))
    keys = {n: [key for key in table if n.startswith(key)] for n in names}
    assert not [n for n in names if len(keys[n]) != 1], {n: k for n, k in keys.items() if len(k) != 1}   # no kernel left over or claimed twice
    built = {key: len([n for n in names if keys[n] == [key]]) for key in table}
    assert built == table, {key: (built[key], table[key]) for key in table if built[key] != table[key]}


def test_scan_kernels_have_no_second_home():
    holders = [i for i, obj in enumerate(inv.objects()) if any(n.startswith("scan_") for n in obj)]
    assert 1 <= len(holders) <= inv.SCAN_OBJECTS, holders
    # no other name hides a second kernel either: what two code objects both hold, both of msm.hip's objects hold
    shared = [{n for n in obj if sum(n in other for other in inv.objects()) > 1} for obj in inv.objects()]
    assert len([s for s in shared if s]) == 2 and len({frozenset(s) for s in shared if s}) == 1, shared
