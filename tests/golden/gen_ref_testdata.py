#!/usr/bin/env python3
"""Copies the reference's own DATA fixtures that tests used to read from a checkout of the reference tree into one compressed archive,
so that those tests run on every machine (test infrastructure; no source code is copied):

    python3 tests/golden/gen_ref_testdata.py <reference tree>  ->  tests/golden/ref_testdata.tar.xz

  <ledgersData.zip path>/<member>   the block files of the sample ledgers gen_ledger_block_fixtures.py reads (its SOURCES), the
                                    archives' only members it looks at
                                    (test_ledger_goldens.py::test_fixture_file_is_what_the_generator_extracts_from_the_reference)
  orderer/.../mychannel.block       the orderers' marshalled config blocks
                                    (test_block_prepass.py::test_block_walker_on_the_reference_block_fixtures)
  certs/<sha256>.der                the first certificate of every *.pem of the tree that ref_cert_chains.json does not already hold
                                    (test_block_prepass.py::test_x509_key_extraction_equals_openssl_on_the_reference_certificates)
"""
import base64
import glob
import hashlib
import io
import json
import lzma
import os
import re
import sys
import tarfile
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_ledger_block_fixtures as ledgers   # noqa: E402

BLOCK_FILES = ["orderer/common/cluster/testdata/mychannel.block", "orderer/consensus/etcdraft/testdata/mychannel.block"]


def first_certificate(raw):
    m = re.search(rb"-----BEGIN CERTIFICATE-----(.*?)-----END CERTIFICATE-----", raw, re.S)
    return base64.b64decode(b"".join(m.group(1).split()))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    entries = {}
    for _, rel in ledgers.SOURCES:
        zf = zipfile.ZipFile(os.path.join(ref, rel))
        for name in zf.namelist():
            if "/blockfile_" in name:
                entries[rel + "/" + name] = zf.read(name)
    for rel in BLOCK_FILES:
        entries[rel] = open(os.path.join(ref, rel), "rb").read()
    have = json.load(open(os.path.join(HERE, "ref_cert_chains.json")))["certs"]
    for path in glob.glob(os.path.join(ref, "**", "*.pem"), recursive=True):
        raw = open(path, "rb").read()
        if b"BEGIN CERTIFICATE" in raw:
            der = first_certificate(raw)
            if hashlib.sha256(der).hexdigest() not in have:
                entries["certs/%s.der" % hashlib.sha256(der).hexdigest()] = der
    out = os.path.join(HERE, "ref_testdata.tar.xz")
    with tarfile.open(out, "w:xz", preset=9 | lzma.PRESET_EXTREME, format=tarfile.USTAR_FORMAT) as tf:
        for name in sorted(entries):                    # fixed order and metadata: the same tree gives the same bytes
            ti = tarfile.TarInfo(name)
            ti.size, ti.mode = len(entries[name]), 0o644
            tf.addfile(ti, io.BytesIO(entries[name]))
    print("%d entries -> %s (%d bytes)" % (len(entries), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
