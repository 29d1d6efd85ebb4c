"""The Go binding (fabric-mod_amd/go/) has never met a compiler - the build image has no Go toolchain.  tools/check_go_sources.py
is the hygiene it gets meanwhile: every file tokenises and balances, every import is used, every reference symbol it names exists in the
reference tree (or in the snapshot taken from it: tests/golden/go_reference_symbols.json), every C.fabgpu_* call matches include/*.h in name
and argument count.  VERDICT r4 item 7."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("check_go_sources", os.path.join(ROOT, "tools", "check_go_sources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_go_binding_is_clean_against_the_reference_or_its_snapshot():
    t = _tool()
    findings, n = t.check(None)                          # the committed snapshot of the reference's declarations
    assert n >= 9 and not findings, "\n".join(findings)


def test_the_benchmarks_the_survey_prefers_exist():
    """SURVEY 8(d) "preferred": bccsp/sw under `go test -bench`, built as the reference's tests build it"""
    src = open(os.path.join(ROOT, "fabric-mod_amd", "go", "bccsp", "gpu", "gpu_bench_test.go")).read()
    for name in ("BenchmarkSWVerify", "BenchmarkSWVerifyParallel", "BenchmarkPreVerifyBlock", "BenchmarkVerifyFromMemo"):
        assert "func %s(b *testing.B)" % name in src
    assert "sw.NewDefaultSecurityLevelWithKeystore(sw.NewDummyKeyStore())" in src
    assert "b.Elapsed()" not in src                      # Go 1.20; the reference builds with Go 1.14 (Makefile:79)


def test_the_checker_catches_what_it_is_for(tmp_path):
    t = _tool()
    toks, errs = t.lex('package x\nfunc f() { g(1, "a)" }\n', "t.go")
    assert not errs and t.balance(toks, "t.go")                                # the ")" inside the string does not close the call
    toks, errs = t.lex("package x\nvar s = `raw\n) string`\nfunc f() {}\n", "t.go")
    assert not errs and not t.balance(toks, "t.go")
    assert t.lex('package x\nvar s = "unterminated\n', "t.go")[1]
    toks, _ = t.lex('package x\nimport (\n\t"fmt"\n\tm "github.com/hyperledger/fabric/common/metrics"\n)\nfunc f() { fmt.Println(m.Provider(nil)) }\n', "t.go")
    assert t.imports_of(toks) == {"fmt": "fmt", "m": "github.com/hyperledger/fabric/common/metrics"}
    uses, sig = t.qualified_uses(toks)
    assert {(q, n) for q, n, _, _ in uses} == {("fmt", "Println"), ("m", "Provider")}
    # arity of a cgo call, nested calls and composite literals inside the arguments
    toks, _ = t.lex("package x\nfunc f() { C.fabgpu_a(p.csp, (*C.uint8_t)(unsafe.Pointer(&b[0])), C.size_t(len(b)), []int{1, 2}) ; C.fabgpu_b() }\n", "t.go")
    uses, sig = t.qualified_uses(toks)
    ar = {n: t.call_arity(sig, k + 2) for q, n, _, k in uses if q == "C" and n.startswith("fabgpu_")}
    assert ar == {"fabgpu_a": 4, "fabgpu_b": 0}
    protos, macros = t.c_prototypes()
    assert protos["fabgpu_strerror"] == 1 and protos["fabgpu_csp_block_pass_abandon"] == 1 and protos["fabgpu_multi_collective"] == 3
    assert "FABGPU_ETOOBIG" in macros and "FABGPU_PASS_SEED_MEMO" in macros
    # exported declarations of a package: top-level funcs, types, grouped declarations; no methods, no unexported names, no _test.go files
    (tmp_path / "impl.go").write_text("package sw\n\ntype CSP struct{ ks KeyStore }\n\ntype (\n\tKeyStore interface{}\n\tdummy    struct{}\n)\n\n"
                                      "func NewDefaultSecurityLevelWithKeystore(ks KeyStore) (*CSP, error) { return &CSP{ks}, nil }\n\n"
                                      "func NewDummyKeyStore() KeyStore { return dummy{} }\n\nfunc verifyECDSA() bool { return false }\n\n"
                                      "func (c *CSP) Verify() bool { return verifyECDSA() }\n")
    (tmp_path / "impl_test.go").write_text("package sw\n\nfunc NewTestCSP() *CSP { return nil }\n")
    names = t.exported_names(str(tmp_path))
    assert names == {"NewDefaultSecurityLevelWithKeystore", "NewDummyKeyStore", "CSP", "KeyStore"}
