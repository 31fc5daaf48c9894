"""CPU tier: the container walk of a serialized proving key (g16_host_pk_bytes_layout, the first thing g16_pk_load_bytes does): the
twelve sections' counts and the bytes consumed on an honest key, and every way the bytes can end early or lie about a length --
refused with G16_ERR_BAD_LENGTH and reason 4 before anything would be allocated."""
import ctypes as C
import struct

import pytest

import pymodel as pm
from key_bytes_cases import VECS, section_offsets
from subgroup_cases import NAMES

import groth16_amd as g
import groth16_amd.serialize as ser
from groth16_amd.binding import PK_BYTES_SECTIONS, PkBytesInfoC

OK, BAD_LENGTH, BAD_ARG = 0, 2, 3


def layout(name, data, compressed, size=None):
    info = PkBytesInfoC()
    rc = g.lib().c.g16_host_pk_bytes_layout(g.CURVE_ID[name], data, len(data), int(compressed), C.byref(info),
                                            C.sizeof(info) if size is None else size)
    return rc, info


@pytest.fixture(scope="module")
def keys(orc):
    out = {}
    for name in NAMES:
        ck = orc.syn_circuit(name, 4, 2)
        pk, ex = orc.setup(ck, 3)
        key = g.ProvingKey(name, pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query, pk.b_g1_query, pk.b_g2_query,
                           pk.h_query, pk.l_query, ex["gamma_g2"][None, :], ex["gamma_abc"])
        for compressed in (True, False):
            out[(name, compressed)] = (ck, ser.proving_key_to_bytes(name, key, compressed))
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False])
def test_counts_and_consumed(keys, name, compressed):
    ck, data = keys[(name, compressed)]
    offs, total = section_offsets(name, ck, compressed)
    L, n, nv, ni = pm.CURVES[name].fq_limbs64 * 8, ck.domain_size, ck.num_vars, ck.num_inputs
    g1s, g2s = (L, 2 * L) if compressed else (2 * L, 4 * L)
    assert total == len(data) == (3 + ni + 2 * nv + (n - 1) + (nv - ni)) * g1s + (3 + nv) * g2s + 6 * 8   # test_proving_key_round_trip's
    rc, info = layout(name, data, compressed)
    assert rc == OK and info.consumed == len(data) and info.bad_section == -1 and info.n_bad == 0
    assert info.counts() == {sec: offs[sec][3] for sec in PK_BYTES_SECTIONS}
    # trailing bytes are not an error; consumed says what was read
    rc, info = layout(name, data + b"\xff" * 13, compressed)
    assert rc == OK and info.consumed == len(data) and info.bad_section == -1
    # a caller with a shorter struct gets no more than it asked for
    rc, short = layout(name, data, compressed, size=8)
    assert rc == OK and short.consumed == len(data) and all(c == 0 for c in short.count) and short.bad_section == 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False])
def test_truncation_and_bad_lengths(keys, name, compressed):
    ck, data = keys[(name, compressed)]
    offs, total = section_offsets(name, ck, compressed)

    def refused(blob, section):
        rc, info = layout(name, blob, compressed)
        assert rc == BAD_LENGTH, (section, rc)
        assert PK_BYTES_SECTIONS[info.bad_section] == section and info.bad_reason == 4, (section, info.bad_section, info.bad_reason)
        assert info.consumed == 0 and info.bad_index == 0 and info.n_bad == 0
        return info

    refused(data[:-1], "l_query")
    refused(b"", "alpha_g1")
    for sec in VECS:
        at, first, size, count = offs[sec]
        refused(data[:at + 3], sec)                                  # inside the length word
        refused(data[:first + (count // 2) * size + size // 2], sec)   # in the middle of a point in the middle of the section
        huge = data[:at] + struct.pack("<Q", 1 << 61) + data[at + 8:]   # 2^61 points of 32 bytes and more: the product wraps
        assert refused(huge, sec).count[PK_BYTES_SECTIONS.index(sec)] == 1 << 61
        refused(data[:at] + struct.pack("<Q", (1 << 64) - 1) + data[at + 8:], sec)
        one_more = data[:at] + struct.pack("<Q", count + 1) + data[at + 8:]
        if sec == "l_query":
            refused(one_more, sec)   # the last section: one point more than the bytes hold
    for sec in ("beta_g2", "delta_g1"):
        refused(data[:offs[sec][1] + 5], sec)


def test_null_context_and_bad_arguments(keys):
    lb = g.lib()
    _, data = keys[("bn254", True)]
    info, handle = PkBytesInfoC(), C.c_void_p(0xDEAD)
    assert lb.c.g16_pk_load_bytes(None, data, len(data), 1, 2, C.byref(handle), C.byref(info), C.sizeof(info)) == BAD_ARG
    assert handle.value is None   # *out is NULL after every refusal
    assert lb.c.g16_host_pk_bytes_layout(2, data, len(data), 1, C.byref(info), C.sizeof(info)) == BAD_ARG
    assert lb.c.g16_host_pk_bytes_layout(1, data, len(data), 2, C.byref(info), C.sizeof(info)) == BAD_ARG
    assert lb.c.g16_host_pk_bytes_layout(1, None, 5, 1, C.byref(info), C.sizeof(info)) == BAD_ARG
    assert lb.c.g16_host_pk_bytes_layout(1, data, len(data), 1, None, 0) == OK
    assert lb.c.g16_struct_size(10) == 0   # g16_pk_bytes_info is sized by its callers, not registered
