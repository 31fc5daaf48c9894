"""CPU tier: every built library holds exactly the kernels tests/kernel_inventory.py lists -- each kernel under exactly one key, each
key's count exact, nothing left over -- and the `static` scan kernels, which every code object that includes them would carry under
the same name, are in msm_sort.hip's object only; no kernel of any library is built twice under one name."""
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
    assert len(holders) == 1, holders
    # no other name hides a second kernel either: no two code objects of a library hold a kernel of one name
    for libname in sorted(inv.INVENTORY):
        objs = inv.objects(libname)
        twice = sorted(n for i, obj in enumerate(objs) for n in obj if any(n in other for other in objs[i + 1:]))
        assert not twice, (libname, twice)
