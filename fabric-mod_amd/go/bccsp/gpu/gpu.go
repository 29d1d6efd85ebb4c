// +build fabgpu

// Package gpu is the reference-side binding of libfabgpu.so: a bccsp.BCCSP that embeds bccsp/sw exactly the
// way bccsp/pkcs11/pkcs11.go:35-52 does and overrides KeyImport (to REMEMBER X, Y under the key's SKI) and Verify.
// Every key it hands out is bccsp/sw's own key object: bccsp/sw dispatches on reflect.TypeOf(key) (bccsp/sw/impl.go:110
// KeyDeriv, :232 Sign, :259 Verify, :296 Decrypt; the registrations are bccsp/sw/new.go:60-96), so a wrapper type around a
// public key would make every verb this provider does not override fail with "Unsupported 'Key' provided" - round 2's
// *gpuPublicKey did exactly that to KeyDeriv (a KeyDeriver IS registered for *ecdsaPublicKey, new.go:86).
//
// Drop this directory into the reference tree as bccsp/gpu and build the peer with GO_TAGS=fabgpu
// (same mechanism as the pkcs11 tag, Makefile:80,209).  Written for the reference's Go 1.14.4 (Makefile:79):
// no big.Int.FillBytes, no generics.  NOT compiled in this repository - the build image has no Go toolchain
// (`go version`: not found); the C ABI it binds is exercised by the Python/ctypes tests instead, and every
// function here is a thin translation of a C call whose behaviour those tests pin.
//
// How the provider earns its keep (SURVEY.md 8(f) rank 1):
//   1. extensions/validation wraps the channel's validator (preverify.go in this delivery): before the unchanged
//      v14/v20 validator runs, the whole marshalled block goes to PreVerifyBlock - ONE device submission for every
//      creator, endorsement and orderer signature of the block, which also seeds the verdict memo inside
//      libfabgpu.so, keyed on (public key, signature bytes, digest the DEVICE computed).
//   2. the validators then call identity.Verify per signature as before (msp/identities.go:169-196):
//      bccsp.Hash finds the digest the pass computed in the library's DIGEST MEMO - handed out only when every byte of
//      the validator's message equals the bytes the device hashed, so the digest still ties the caller's bytes to the
//      memo entry (a miss: bccsp/sw hashes on the CPU) - and bccsp.Verify finds the verdict in the verdict memo.  A miss,
//      a non-P-256 key, or any rejected signature goes to bccsp/sw, so error text and semantics are the reference's own
//      in every case but "valid".
//   3. when Validate returns, the wrapper evicts the block's entries: the memo never grows with the chain.
// The device never decides alone: a verdict is only ever attached to the three byte strings the validator itself
// presents, so a block whose bytes the pass parsed differently than the Go unmarshaller (or a device failure)
// can only produce misses.
package gpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../lib -lfabgpu
#include <stdlib.h>
#include <string.h>
#include "fabgpu.h"
#include "fabgpu_bccsp.h"

// cgo pointer rule: Go memory handed to C must not itself contain Go pointers, so the descriptor struct (which points at the
// block and at the flags array, both Go memory) is built on the C stack here, from plain arguments.
static int fabgpu_go_block_pass(fabgpu_csp* csp, const uint8_t* block, size_t len, uint64_t seq, uint32_t flags, uint8_t* tx_flags,
                                uint32_t cap_tx, uint32_t cap_tuples, uint32_t* n_tx, uint32_t* n_tuples, uint32_t* n_block_sigs,
                                uint32_t* memo_seeded) {
    fabgpu_block_pass ps;
    memset(&ps, 0, sizeof(ps));
    ps.block = block;
    ps.len = len;
    ps.block_seq = seq;
    ps.flags = flags;
    ps.cap_tx = cap_tx;
    ps.cap_tuples = cap_tuples;
    ps.tx_flags = tx_flags;
    int rc = fabgpu_csp_block_preverify2(csp, &ps);
    *n_tx = ps.n_tx;
    *n_tuples = ps.n_tuples;
    *n_block_sigs = ps.n_block_sigs;
    *memo_seeded = ps.memo_seeded;
    return rc;
}
*/
import "C"

import (
	"crypto/ecdsa"
	"crypto/elliptic"
	"crypto/x509"
	"math/big"
	"strconv"
	"sync"
	"sync/atomic"
	"time"
	"unsafe"

	"github.com/hyperledger/fabric/bccsp"
	"github.com/hyperledger/fabric/common/metrics"
	"github.com/pkg/errors"
)

// Provider is the concrete type behind the bccsp.BCCSP that New returns; extensions/validation type-asserts for
// BlockPreVerifier to find out whether the default BCCSP can pre-verify blocks.
type Provider struct {
	bccsp.BCCSP // bccsp/sw: everything that is not overridden (pattern: bccsp/pkcs11/pkcs11.go:35-37)
	csp         *C.fabgpu_csp
	closeOnce   sync.Once
	keys        keyXY
	inflight    sync.Map // blockSeq -> chan struct{}: passes that are running right now (arrival hook / validator wrapper)
	// coalesce: memo misses go to the device through fabgpu_csp_verify_coalesced instead of straight to bccsp/sw - for
	// processes whose Verify calls arrive many at a time on their own goroutines and no block pass sees them first: the
	// orderer (Broadcast handlers behind SigFilter, orderer/common/msgprocessor/sigfilter.go:50-80).  Off by default: a
	// lone call costs a launch (0.7 ms) where bccsp/sw costs 0.1 ms; the break-even is about sixteen calls in flight.
	coalesce bool
	// p384: Options.P384 - Verify on a P-384 key asks the P-384 verdict memo (fabgpu_csp_memo_lookup_p384) and, on a miss, the device
	// (fabgpu_csp_verify_coalesced_p384) before bccsp/sw; keys384 remembers the
	// coordinates of the P-384 public keys KeyImport has seen, by SKI (string(ski) -> *[96]byte); each is registered on the device once
	// (fabgpu_csp_key_import_p384)
	p384    bool
	keys384 sync.Map
	// noHashMemo: Options.NoHashMemo - Hash goes straight to bccsp/sw
	noHashMemo bool
	// poisoned (atomic, 0 / 1): the library's CPU audit disagreed with the device once (Options.AuditPermille; fabgpu_bccsp.h "CPU
	// audit") and the library answers FABGPU_EPOISONED / misses for good.  Set when a call returns FABGPU_EPOISONED or the metrics
	// refresher sees the flag; from then on no call crosses cgo any more: Hash, Verify and everything else is the embedded bccsp/sw's,
	// PreVerifyBlock returns an error (validation proceeds on bccsp/sw) and HasBlock answers false.  Never cleared: the peer is
	// restarted after whoever runs it has looked at the reason (PoisonedReason; the library also prints it to stderr).
	poisoned uint32
	// room for per-transaction flags, remembered from block to block (atomic max): the library answers FABGPU_ETOOBIG - nothing was
	// launched, the upload has been waited for (the library never reads the block after a call returned) and is kept for the retry,
	// which finds it again - only when a block outgrows every block before it
	capTx uint32
	// metrics: published through an atomic.Value (RegisterMetrics may run while PreVerifyBlock goroutines are already reading it);
	// the refresher goroutine is stopped by Close BEFORE the C provider is freed (ADVICE r4)
	mv          atomic.Value // *passMetrics; empty until RegisterMetrics
	metricsOnce sync.Once
	stopMetrics chan struct{}
	metricsDone chan struct{}
}

// metrics returns the registered pass metrics, or nil (every passMetrics method is nil-safe)
func (p *Provider) metrics() *passMetrics {
	m, _ := p.mv.Load().(*passMetrics)
	return m
}

// Options is what GPUFactory reads from the `GPU:` section of the BCCSP configuration (bccsp/factory/gpufactory.go GPUOpts) - the
// fabgpu_csp_opts of include/fabgpu_bccsp.h.  The reference has ONE process-global BCCSP (bccsp/factory/factory.go:41-55) that every
// channel's validator shares (core/peer/peer.go:337-355): it owns every device listed here and spreads the block passes over them.
type Options struct {
	Devices          []int // HIP ordinals, one device context each (an ordinal may repeat); empty: every visible device
	ConcurrentPasses int   // per device: staging slots, pinned memo tables and pass arrays for that many overlapping passes are allocated now
	ExpectBlockBytes int   // sizes that pre-allocation (0: 64 MiB) ...
	ExpectTuples     int   // ... (0: 65 536 signatures per block)
	MemoBlocks       int   // the verdict memo holds this many blocks' worth of entries (x ExpectTuples); 0: the library's 2^18 entries
	NoHashMemo       bool  // bccsp.Hash never asks the digest memo and passes keep no host copy of their block (default: they do)
	HashMemoBlocks   int   // per device: host copies of blocks kept for the digest memo at a time (0: MemoBlocks + ConcurrentPasses, at least 8)
	KeyTables16      bool  // FABGPU_FLAG_KEY_TABLES_16BIT: every imported key also gets a 16-bit comb table on the device (80 MiB each, the first 64 keys)
	HostWalk         bool  // keep the envelope walk on the host (A/B runs)
	PassTiming       bool  // stage breakdown of every pass on stderr
	// AuditPermille (0 .. 1000): the library re-computes this share of the digests and verdicts it is about to hand out from the device
	// on the CPU first - digest-memo hits, verdict-memo hits of P-256 entries, "valid" answers of the coalesced Verify - and poisons
	// the provider at the first disagreement (hit h of a kind is audited iff h*permille/1000 != (h-1)*permille/1000: no randomness).
	// GPUFactory passes 1 unless the operator says otherwise; 0 switches the audit off.  Idemix pseudonym results are a sampled kind of
	// their own (NymAuditStats).
	AuditPermille int
	// RetireEvictedKeys: identities the identity cache evicts give their device comb tables up (option "retire_evicted_keys";
	// KeyTableStats, gauges bccsp_gpu_key_tables).  GPUFactory passes true unless the operator says otherwise.
	RetireEvictedKeys bool
	// SHA3: the library serves the SHA3 hash family on the device (option "hash_sha3"): batched identity verification of an MSP whose
	// SignatureHashFamily is SHA3 (fabgpu_csp_identity_verify_batch2 / _coalesced2 with family "SHA3").  One-message Hash calls stay with
	// bccsp/sw whatever this says (Provider.Hash).  Not served: the block pass, which hashes with SHA-256 - a SHA3 MSP's signatures come
	// back "not valid" from it and are decided by bccsp/sw.  GPUFactory passes true unless the operator says otherwise.
	SHA3 bool
	// P384: Verify on an ECDSA P-384 key (bccsp/sw accepts them exactly as P-256 keys, bccsp/sw/keyimport.go, ecdsa.go:41-57) goes to the
	// device through fabgpu_csp_verify_coalesced_p384 (option "p384") and takes only "valid" from it; everything else, and every error
	// text, stays bccsp/sw's.  False (the default, also GPUFactory's): a P-384 key flows through untouched, and the block pass
	// leaves a P-384 creator or endorser TX_NEEDS_SW.  True: the pass verifies them too (its P-384 stage, fabgpu_csp_p384_pass_stats) and
	// the transaction's flag says so, and a memo-seeding pass remembers their verdicts in a memo of their own: Verify below asks
	// fabgpu_csp_memo_lookup_p384 first and the coalesced entry only on a miss.  bccsp.Hash of their messages stays bccsp/sw's.
	P384 bool
	// P384Wide: FABGPU_FLAG_P384_WIDE on every context - keyed P-384 launches of at most 8 192 rows run with eight lanes per signature
	// (a 1 000-transaction P-384 block is 4 000 rows: a sixteenth of what fills the chip one signature per lane).  False by default.
	P384Wide bool
	// P384KeyTables16: FABGPU_FLAG_P384_KEY_TABLES_16BIT on every context - each imported P-384 key also gets a 16-bit comb table
	// (144 MiB, at most 32 per context), and keyed launches run 24 windows of two additions on the wavefronts all of whose keys have
	// one.  False by default.  Verdicts do not depend on it.
	P384KeyTables16 bool
	// SHA3Coop: FABGPU_FLAG_SHA3_COOP on every context - SHA3-256 launches of at most 4 096 messages run with 32 lanes on a message, and
	// larger plain launches hash their few long messages that way.  False by default.  Digests and verdicts do not depend on it.
	SHA3Coop bool
}

// SetCoalesce switches the coalesced device path for memo misses on or off (GPUOpts.CoalesceVerify in gpufactory.go).
func (p *Provider) SetCoalesce(on bool) { p.coalesce = on }

// BlockPreVerifier is what the validator wrapper needs from the default BCCSP.
type BlockPreVerifier interface {
	// PreVerifyBlock submits every signature of the marshalled block to the device and seeds the verdict memo under
	// blockSeq.  A non-nil error is an infrastructure failure: the caller ignores it and validation proceeds on bccsp/sw.
	PreVerifyBlock(blockBytes []byte, blockSeq uint64) (*PassSummary, error)
	// EvictBlock drops the memo entries seeded under blockSeq.
	EvictBlock(blockSeq uint64)
	// HasBlock: a pass under blockSeq has already seeded the memo (the arrival hook ran) and nothing evicted it since.
	HasBlock(blockSeq uint64) bool
}

// PassSummary is the per-transaction advice of one pass (never consensus input: the validators decide).
type PassSummary struct {
	TxFlags    []uint8 // fabgpu_bccsp.h: 0 all signatures valid, 1 bad creator signature, 2 bad endorsement, 3 not understood, 4 needs bccsp/sw, 5 TxID mismatch, 6 proposal-hash mismatch
	Tuples     int
	BlockSigs  int
	MemoSeeded int
}

// keyXY remembers the affine coordinates of every on-curve P-256 public key this provider imported, under the key's SKI
// (bccsp/sw/ecdsakey.go:87-99: SHA-256 of the uncompressed point - the same for a private key and its public half), so that
// Verify never needs the unexported sw key type (bccsp/sw/ecdsakey.go:72-74) and never has to wrap it either.  Two generations:
// when the young one is full it becomes the old one and the old one is dropped; a key that is still in use is found in the old
// generation and moves back.  A key that fell out (imported long ago, never verified with since) just verifies on bccsp/sw.
type keyXY struct {
	mu         sync.RWMutex
	young, old map[string][64]byte
}

const keyXYGeneration = 1 << 16 // entries per generation (an entry: 32-byte SKI + 64 bytes)

func (s *keyXY) put(ski []byte, xy *[64]byte) {
	s.mu.Lock()
	if s.young == nil {
		s.young = make(map[string][64]byte)
	}
	if len(s.young) >= keyXYGeneration {
		s.old, s.young = s.young, make(map[string][64]byte)
	}
	s.young[string(ski)] = *xy
	s.mu.Unlock()
}

func (s *keyXY) get(ski []byte) (xy [64]byte, ok bool) {
	s.mu.RLock()
	xy, ok = s.young[string(ski)]
	inOld := false
	if !ok {
		xy, inOld = s.old[string(ski)]
	}
	s.mu.RUnlock()
	if inOld {
		s.put(ski, &xy)
		return xy, true
	}
	return xy, ok
}

// New is what bccsp/factory calls for ProviderName "GPU" (gpufactory.go): ONE provider over every device of opts.Devices.
func New(swCSP bccsp.BCCSP, opts Options) (bccsp.BCCSP, error) {
	if swCSP == nil {
		return nil, errors.New("Invalid software BCCSP. It must not be nil.")
	}
	var o C.fabgpu_csp_opts // zeroed: every switch at its default
	o.size = C.uint32_t(unsafe.Sizeof(o))
	o.n_devices = C.int32_t(len(opts.Devices))
	var devs *C.int32_t
	if len(opts.Devices) != 0 { // the ordinals live in C memory for the call (cgo: no Go pointer inside a struct handed to C)
		devs = (*C.int32_t)(C.malloc(C.size_t(4 * len(opts.Devices))))
		defer C.free(unsafe.Pointer(devs))
		arr := (*[1 << 16]C.int32_t)(unsafe.Pointer(devs))
		for i, d := range opts.Devices {
			arr[i] = C.int32_t(d)
		}
		o.devices = devs
	}
	o.concurrent_passes = C.uint32_t(opts.ConcurrentPasses)
	o.expect_block_bytes = C.uint64_t(opts.ExpectBlockBytes)
	o.expect_tuples = C.uint32_t(opts.ExpectTuples)
	if opts.KeyTables16 {
		o.ctx_flags |= 256 // fabgpu.h FABGPU_FLAG_KEY_TABLES_16BIT
	}
	if opts.P384Wide {
		o.ctx_flags |= 4096 // fabgpu.h FABGPU_FLAG_P384_WIDE
	}
	if opts.P384KeyTables16 {
		o.ctx_flags |= 8192 // fabgpu.h FABGPU_FLAG_P384_KEY_TABLES_16BIT
	}
	if opts.SHA3Coop {
		o.ctx_flags |= 32768 // fabgpu.h FABGPU_FLAG_SHA3_COOP
	}
	if opts.HostWalk {
		o.pass_device_walk = -1
	}
	if opts.PassTiming {
		o.pass_timing = 1
	}
	if opts.NoHashMemo {
		o.pass_hash_memo = -1
	}
	// a block's host copy lives as long as its memo entries: as many copies as blocks may wait for their validators, plus the passes in flight
	keep := opts.HashMemoBlocks
	if keep <= 0 {
		keep = opts.MemoBlocks + opts.ConcurrentPasses
		if keep < 8 {
			keep = 8
		}
	}
	if keep > 64 {
		keep = 64
	}
	o.hash_memo_blocks = C.uint32_t(keep)
	if opts.AuditPermille < 0 || opts.AuditPermille > 1000 {
		return nil, errors.Errorf("Invalid GPU opts: AuditPermille [%d] must be 0 .. 1000", opts.AuditPermille)
	}
	o.audit_permille = C.uint32_t(opts.AuditPermille)
	var csp *C.fabgpu_csp
	errbuf := make([]byte, 256)
	if rc := C.fabgpu_csp_new2(&o, &csp, (*C.char)(unsafe.Pointer(&errbuf[0])), C.size_t(len(errbuf))); rc != 0 {
		return nil, errors.Errorf("Failed initializing GPU BCCSP: %s (%s)", C.GoString(C.fabgpu_strerror(rc)), C.GoString((*C.char)(unsafe.Pointer(&errbuf[0]))))
	}
	if opts.RetireEvictedKeys {
		name := C.CString("retire_evicted_keys")
		rc := C.fabgpu_csp_set_option(csp, name, 1, nil)
		C.free(unsafe.Pointer(name))
		if rc != 0 {
			C.fabgpu_csp_free(csp)
			return nil, errors.Errorf("Failed initializing GPU BCCSP: retire_evicted_keys: %s", C.GoString(C.fabgpu_strerror(rc)))
		}
	}
	if opts.SHA3 {
		name := C.CString("hash_sha3")
		rc := C.fabgpu_csp_set_option(csp, name, 1, nil)
		C.free(unsafe.Pointer(name))
		if rc != 0 {
			C.fabgpu_csp_free(csp)
			return nil, errors.Errorf("Failed initializing GPU BCCSP: hash_sha3: %s", C.GoString(C.fabgpu_strerror(rc)))
		}
	}
	if opts.P384 {
		name := C.CString("p384")
		rc := C.fabgpu_csp_set_option(csp, name, 1, nil)
		C.free(unsafe.Pointer(name))
		if rc != 0 {
			C.fabgpu_csp_free(csp)
			return nil, errors.Errorf("Failed initializing GPU BCCSP: p384: %s", C.GoString(C.fabgpu_strerror(rc)))
		}
	}
	if opts.MemoBlocks > 0 {
		// (peer.gossip.state.blockBufferSize blocks may be waiting for their validators: the memo must hold them all, or it drops the
		// oldest - the block the committer needs next - and every block of a catch-up is passed twice)
		tuples := opts.ExpectTuples
		if tuples <= 0 {
			tuples = 65536
		}
		C.fabgpu_csp_memo_set_capacity(csp, C.uint64_t(opts.MemoBlocks)*C.uint64_t(tuples))
	}
	// room for per-transaction flags to start with: a block has fewer transactions than signatures, so an operator who sized the
	// provider (ExpectTuples) has already said how large it needs to be - the first big block then costs no FABGPU_ETOOBIG round trip
	capTx := uint32(1024)
	if opts.ExpectTuples > 1024 {
		capTx = uint32(opts.ExpectTuples)
	}
	return &Provider{BCCSP: swCSP, csp: csp, capTx: capTx, noHashMemo: opts.NoHashMemo, p384: opts.P384}, nil
}

// Devices: how many device contexts this provider drives.
func (p *Provider) Devices() int { return int(C.fabgpu_csp_device_count(p.csp)) }

// PassesPerDevice: block passes each device context has served (metrics).
func (p *Provider) PassesPerDevice() []uint64 {
	n := p.Devices()
	if n <= 0 {
		return nil
	}
	v := make([]C.uint64_t, n)
	if int(C.fabgpu_csp_passes_per_device(p.csp, &v[0], C.int(n))) != n {
		return nil
	}
	out := make([]uint64, n)
	for i := range v {
		out[i] = uint64(v[i])
	}
	return out
}

// Close releases the device context (tests; a peer keeps its BCCSP for life).
func (p *Provider) Close() {
	p.closeOnce.Do(func() {
		// the metrics refresher calls into the C provider: it must be gone before the provider is
		p.metricsOnce.Do(func() {}) // (no refresher may be started from here on)
		if p.stopMetrics != nil {
			close(p.stopMetrics)
			<-p.metricsDone
		}
		C.fabgpu_csp_free(p.csp)
	})
}

// Poisoned: the library's CPU audit found the device disagreeing with the CPU (or the library was poisoned by hand) and this provider
// serves everything from the embedded bccsp/sw from now on.
func (p *Provider) Poisoned() bool {
	if atomic.LoadUint32(&p.poisoned) != 0 {
		return true
	}
	if C.fabgpu_csp_poisoned(p.csp, nil, 0) == 1 {
		p.markPoisoned()
		return true
	}
	return false
}

// PoisonedReason: the first reason the library was poisoned for ("" while it is not).
func (p *Provider) PoisonedReason() string {
	why := make([]byte, 512)
	if C.fabgpu_csp_poisoned(p.csp, (*C.char)(unsafe.Pointer(&why[0])), C.size_t(len(why))) != 1 {
		return ""
	}
	n := 0
	for n < len(why) && why[n] != 0 {
		n++
	}
	return string(why[:n])
}

// markPoisoned is the switch to bccsp/sw: after it no method of the provider calls into the library's lookups, verifies or passes.
func (p *Provider) markPoisoned() {
	if atomic.CompareAndSwapUint32(&p.poisoned, 0, 1) {
		if m := p.metrics(); m != nil {
			m.poisoned.Set(1)
		}
	}
}

// AuditStats: what the library's CPU audit has done - audits of digest-memo hits, of verdict-memo hits and of direct calls, mismatches
// (the first one poisons), sampled pseudonym results that could not be audited, and the time the audits took on the calling goroutines'
// threads.  (The pseudonym audits themselves: NymAuditStats.)
func (p *Provider) AuditStats() (digest, verdict, direct, mismatches, skippedNym uint64, spent time.Duration) {
	var v [6]C.uint64_t
	if C.fabgpu_csp_audit_stats(p.csp, &v[0], 6) != 6 {
		return
	}
	return uint64(v[0]), uint64(v[1]), uint64(v[2]), uint64(v[3]), uint64(v[4]), time.Duration(v[5])
}

// NymAuditStats: the idemix pseudonym results the CPU audit verified again (memo hits of pseudonym entries and "valid" answers of the
// nym batch - the library's seventh counter), and the sampled ones it could not audit: the block copy with the message was no longer
// held, or the issuer's fields were not at hand.
func (p *Provider) NymAuditStats() (audits, skipped uint64) {
	var v [7]C.uint64_t
	if C.fabgpu_csp_audit_stats(p.csp, &v[0], 7) != 7 {
		return
	}
	return uint64(v[6]), uint64(v[4])
}

// KeyTableStats: the registered keys' tables on device context d - keys live, slots draining behind a retirement, registrations that
// reused a retired slot, slots parked for good, bytes of device memory held - and the keys this provider has retired for evicted
// identities (fabgpu_csp_key_table_stats).
func (p *Provider) KeyTableStats(d int) (live, draining, reused, parked, bytesHeld, retired uint64) {
	var v [8]C.uint64_t
	if C.fabgpu_csp_key_table_stats(p.csp, C.int(d), &v[0], 8) != 8 {
		return
	}
	return uint64(v[0]), uint64(v[1]), uint64(v[2]), uint64(v[3]), uint64(v[5]), uint64(v[7])
}

// be32 is big.Int.FillBytes for Go 1.14: the value as exactly 32 big-endian bytes (callers guarantee BitLen <= 256).
func be32(v *big.Int, out *[32]byte) {
	b := v.Bytes()
	for i := range out {
		out[i] = 0
	}
	copy(out[32-len(b):], b)
}

// KeyImport owns the public-key import opts so that X, Y are reachable (pattern: bccsp/pkcs11/pkcs11.go:148-179).
// Everything that is not an on-curve P-256 public key is returned exactly as bccsp/sw made it.
func (p *Provider) KeyImport(raw interface{}, opts bccsp.KeyImportOpts) (bccsp.Key, error) {
	k, err := p.BCCSP.KeyImport(raw, opts)
	if err != nil {
		return nil, err
	}
	var pub *ecdsa.PublicKey
	switch opts.(type) {
	case *bccsp.X509PublicKeyImportOpts:
		if cert, ok := raw.(*x509.Certificate); ok {
			pub, _ = cert.PublicKey.(*ecdsa.PublicKey)
		}
	case *bccsp.ECDSAGoPublicKeyImportOpts:
		pub, _ = raw.(*ecdsa.PublicKey)
	}
	if p.p384 && pub != nil && pub.Curve == elliptic.P384() && pub.X != nil && pub.Y != nil {
		// Options.P384: remember an on-curve P-384 key's coordinates for Verify; the key itself stays bccsp/sw's own, as below
		if pub.X.Sign() >= 0 && pub.Y.Sign() >= 0 && pub.X.BitLen() <= 384 && pub.Y.BitLen() <= 384 && pub.Curve.IsOnCurve(pub.X, pub.Y) {
			var xy [96]byte
			bx, by := pub.X.Bytes(), pub.Y.Bytes() // (no big.Int.FillBytes in Go 1.14; BitLen <= 384 was checked)
			copy(xy[48-len(bx):48], bx)
			copy(xy[96-len(by):], by)
			if _, seen := p.keys384.LoadOrStore(string(k.SKI()), &xy); !seen {
				// the key's comb table on every device of the pool: Verify's batches then run on the keyed kernel (best effort - a key
				// without a table is served by the fresh-key kernel, with the same answers)
				C.fabgpu_csp_key_import_p384(p.csp, (*C.uint8_t)(unsafe.Pointer(&xy[0])), (*C.uint8_t)(unsafe.Pointer(&xy[48])), nil, nil, 0)
			}
		}
		return k, nil
	}
	if pub == nil || pub.Curve != elliptic.P256() || pub.X == nil || pub.Y == nil {
		return k, nil // not ours: sw handles it
	}
	if pub.X.Sign() < 0 || pub.Y.Sign() < 0 || pub.X.BitLen() > 256 || pub.Y.BitLen() > 256 || !pub.Curve.IsOnCurve(pub.X, pub.Y) {
		return k, nil // ECDSAGoPublicKeyImportOpts does not check the point (bccsp/sw/keyimport.go:103-112): such keys stay with sw
	}
	var xy [64]byte
	var x, y [32]byte
	be32(pub.X, &x)
	be32(pub.Y, &y)
	copy(xy[:32], x[:])
	copy(xy[32:], y[:])
	p.keys.put(k.SKI(), &xy)
	return k, nil // bccsp/sw's own key: every other verb of bccsp/sw keeps working on it
}

// xyOf: the coordinates this provider remembered for k's SKI (public and private ECDSA keys share it; bccsp/sw verifies with a
// private key's public half, bccsp/sw/ecdsa.go:59-69, and so does the memo).
func (p *Provider) xyOf(k bccsp.Key) (xy [64]byte, ok bool) {
	if k == nil || k.Symmetric() {
		return xy, false
	}
	ski := k.SKI()
	if len(ski) == 0 {
		return xy, false
	}
	return p.keys.get(ski)
}

// Verify: (true, nil) comes from the verdict memo; every other outcome - and every error text - from bccsp/sw
// (bccsp/sw/impl.go:247-270, ecdsa.go:41-57).  There is deliberately no single-signature device call of its own: one
// launch costs more than one CPU verification.  With SetCoalesce(true) a miss joins whatever other misses are in flight
// (fabgpu_csp_verify_coalesced): the orderer's case.
func (p *Provider) Verify(k bccsp.Key, signature, digest []byte, opts bccsp.SignerOpts) (bool, error) {
	if len(signature) != 0 && len(digest) != 0 && atomic.LoadUint32(&p.poisoned) == 0 {
		if xy, ok := p.xyOf(k); ok {
			var st C.uint8_t
			hit := C.fabgpu_csp_memo_lookup(p.csp, (*C.uint8_t)(unsafe.Pointer(&xy[0])), (*C.uint8_t)(unsafe.Pointer(&xy[32])),
				(*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)),
				(*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &st)
			if hit == 0 && st == C.FABGPU_ST_VALID {
				return true, nil
			}
			if p.coalesce {
				// calls in flight at the same moment share one launch; only "valid" is taken from the device - a reject, a key the
				// device does not decide, or a device failure falls through to bccsp/sw for the reference's own answer and text
				var valid, flags C.int
				var errbuf [8]C.char
				rc := C.fabgpu_csp_verify_coalesced(p.csp, (*C.uint8_t)(unsafe.Pointer(&xy[0])), (*C.uint8_t)(unsafe.Pointer(&xy[32])),
					(*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)),
					(*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &valid, &flags, &errbuf[0], C.size_t(len(errbuf)))
				if rc == 0 && valid == 1 && errbuf[0] == 0 {
					return true, nil
				}
				if rc == C.FABGPU_EPOISONED { // this call's audit failed, or an earlier one: bccsp/sw below, and from now on
					p.markPoisoned()
				}
			}
		}
	}
	if p.p384 && k != nil && !k.Symmetric() && len(signature) != 0 && len(digest) != 0 && atomic.LoadUint32(&p.poisoned) == 0 {
		if v, ok := p.keys384.Load(string(k.SKI())); ok {
			// a P-384 identity (Options.P384): first the verdict memo of the pass's P-384 tuples (fabgpu_csp_memo_lookup_p384; digest is
			// the SHA-256 bccsp/sw just computed - bccsp.Hash of these messages is not served by the digest memo).  Status 0: valid.  A hit
			// with any other status: the pass rejected exactly this tuple - bccsp/sw decides it again and owns the error text, no launch.
			// A miss - no pass seeded it, the block was evicted, a tuple the pass's host gate decided - takes the coalesced entry as
			// before, and only "valid" is taken from it.
			xy := v.(*[96]byte)
			var st C.uint8_t
			hit := C.fabgpu_csp_memo_lookup_p384(p.csp, (*C.uint8_t)(unsafe.Pointer(&xy[0])), (*C.uint8_t)(unsafe.Pointer(&xy[48])),
				(*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)),
				(*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &st, nil)
			if hit == 0 && st == C.FABGPU_ST_VALID {
				return true, nil
			}
			if hit == 0 {
				return p.BCCSP.Verify(k, signature, digest, opts)
			}
			var valid, flags C.int
			var errbuf [8]C.char
			rc := C.fabgpu_csp_verify_coalesced_p384(p.csp, (*C.uint8_t)(unsafe.Pointer(&xy[0])), (*C.uint8_t)(unsafe.Pointer(&xy[48])),
				(*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)),
				(*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &valid, &flags, &errbuf[0], C.size_t(len(errbuf)))
			if rc == 0 && valid == 1 && errbuf[0] == 0 {
				return true, nil
			}
			if rc == C.FABGPU_EPOISONED {
				p.markPoisoned()
			}
		}
	}
	return p.BCCSP.Verify(k, signature, digest, opts) // nil key, foreign key types, misses, rejects: the reference's own answer
}

// (Sign, Encrypt, Decrypt, KeyDeriv, KeyGen, GetKey, GetHashOpt, GetHash are bccsp/sw's, reached through the embedded interface with
// bccsp/sw's own key objects: nothing to unwrap.  INTEGRATION.md lists every bccsp.BCCSP method x key type with who answers.)

// hashMemoMinLen: shorter messages are hashed by bccsp/sw without asking (one SHA-256 block costs less than a cgo call; the library
// answers "miss" for them anyway).
const hashMemoMinLen = 64

// Hash: the `digest, err := id.msp.bccsp.Hash(msg, hashOpt)` half of identity.Verify (msp/identities.go:173-181).  For
// *bccsp.SHA256Opts - what msp/identities.go:216-224 selects for the SHA2 family - the provider first asks the DIGEST MEMO
// (fabgpu_csp_hash_lookup): a block pass that seeded the verdict memo has hashed exactly these bytes on the device and kept the block in
// host memory the library owns; the stored digest comes back ONLY when every byte of msg equals the bytes the device hashed (the
// library compares them all - a fingerprint merely chooses where to look), so the digest is still bound to the validator's own bytes.
// A miss - any other message, an evicted block, a switched-off memo - and every other HashOpts (SHA384, nil: bccsp/sw's error
// text, bccsp/sw/impl.go:179-181) go to bccsp/sw.  So does *bccsp.SHA3_256Opts, also with Options.SHA3 on: the device hashes SHA3-256
// in batches (fabgpu_sha3_256_batch behind the identity batches of a SHA3 MSP), and one launch per message never pays - a 2 KB message
// is a few microseconds of sha3.New256 against a PCIe round trip; the digest memo holds SHA-256 digests only.
// No PCIe round trip either way: a hit is a table probe and a memcmp.
// Before round 6 Hash always went to bccsp/sw: the validators then re-hashed on the CPU every byte the device had just hashed (100 MB
// per 10 000-transaction block), which was three to four times the cost of the GPU pass itself.
func (p *Provider) Hash(msg []byte, opts bccsp.HashOpts) ([]byte, error) {
	if _, isSHA256 := opts.(*bccsp.SHA256Opts); isSHA256 && len(msg) >= hashMemoMinLen && !p.noHashMemo && atomic.LoadUint32(&p.poisoned) == 0 {
		digest := make([]byte, 32)
		if C.fabgpu_csp_hash_lookup(p.csp, (*C.uint8_t)(unsafe.Pointer(&msg[0])), C.size_t(len(msg)), (*C.uint8_t)(unsafe.Pointer(&digest[0]))) == 0 {
			return digest, nil
		}
	}
	return p.BCCSP.Hash(msg, opts)
}

// HashMemoStats is for metrics / tests: bccsp.Hash calls the digest memo answered, calls left to bccsp/sw, host copies of blocks the
// library holds for it right now and their bytes, passes that found the pool of copies exhausted.
func (p *Provider) HashMemoStats() (hits, misses, blocksHeld, bytesHeld, refused uint64) {
	var h, m, b, y, r C.uint64_t
	C.fabgpu_csp_hash_memo_stats(p.csp, &h, &m, &b, &y, &r)
	return uint64(h), uint64(m), uint64(b), uint64(y), uint64(r)
}

// PreVerifyBlock: fabgpu_csp_block_preverify2 with FABGPU_PASS_SEED_MEMO.  blockBytes = proto.Marshal(block).
func (p *Provider) PreVerifyBlock(blockBytes []byte, blockSeq uint64) (*PassSummary, error) {
	if len(blockBytes) == 0 {
		return nil, errors.New("empty block")
	}
	if atomic.LoadUint32(&p.poisoned) != 0 {
		return nil, errors.New("fabgpu: provider poisoned by its CPU audit, validation runs on bccsp/sw")
	}
	// one pass per block name at a time: whoever comes second (the validator wrapper while the arrival hook's pass is still
	// running, a gossiped duplicate) waits for the first and finds the memo seeded
	done := make(chan struct{})
	if other, running := p.inflight.LoadOrStore(blockSeq, done); running {
		<-other.(chan struct{})
		if p.HasBlock(blockSeq) {
			return &PassSummary{}, nil
		}
		return nil, errors.New("fabgpu: the pass this call waited for failed")
	}
	defer func() {
		p.inflight.Delete(blockSeq)
		close(done)
	}()
	// Room for the flags: what the largest block so far needed (atomic max).  No per-tuple array is asked for, so the tuple capacity is
	// not checked at all; FABGPU_ETOOBIG can only mean "more transactions than any block before" - it is decided from the host's outline
	// of the block before anything is launched; the library then waits for the upload it had started (so that it never reads blockBytes
	// after the call returned) and keeps it, and the retry below - same buffer, length and name, bytes unchanged, at once - finds that
	// upload again: growing costs the outline (0.15 ms per 10 000 transactions) and no second transfer, once.
	start := time.Now()
	for attempt := 0; attempt < 3; attempt++ {
		capTx := atomic.LoadUint32(&p.capTx)
		flags := make([]uint8, capTx) // the only array this caller wants back; the memo lives behind the ABI
		var nTx, nTuples, nBlockSigs, seeded C.uint32_t
		rc := C.fabgpu_go_block_pass(p.csp, (*C.uint8_t)(unsafe.Pointer(&blockBytes[0])), C.size_t(len(blockBytes)), C.uint64_t(blockSeq),
			C.FABGPU_PASS_SEED_MEMO, (*C.uint8_t)(unsafe.Pointer(&flags[0])), C.uint32_t(capTx), 0, &nTx, &nTuples, &nBlockSigs, &seeded)
		if rc == C.FABGPU_ETOOBIG { // n_tx is set; nothing was launched, the upload is kept for the retry
			want := uint32(nTx) + uint32(nTx)/8 + 16
			for {
				cur := atomic.LoadUint32(&p.capTx)
				if cur >= want || atomic.CompareAndSwapUint32(&p.capTx, cur, want) {
					break
				}
			}
			continue
		}
		if rc == C.FABGPU_EPOISONED {
			p.markPoisoned()
		}
		if rc != 0 {
			p.metrics().passFailed()
			return nil, errors.Errorf("fabgpu: %s", C.GoString(C.fabgpu_strerror(rc)))
		}
		p.metrics().passDone(time.Since(start), int(nTx), int(nTuples), int(seeded))
		return &PassSummary{TxFlags: flags[:nTx], Tuples: int(nTuples), BlockSigs: int(nBlockSigs), MemoSeeded: int(seeded)}, nil
	}
	C.fabgpu_csp_block_pass_abandon(p.csp) // no retry will come: drop the upload the library kept for one
	p.metrics().passFailed()
	return nil, errors.New("fabgpu: block shape changed between attempts")
}

// EvictBlock: fabgpu_csp_memo_evict_block.
func (p *Provider) EvictBlock(blockSeq uint64) {
	C.fabgpu_csp_memo_evict_block(p.csp, C.uint64_t(blockSeq), nil)
}

// MemoLookup exposes the verdict memo to the other verifier of this delivery (bccsp/idemixgpu: pseudonym signatures are memoised
// under key = Nym.x || Nym.y, digest = SHA-256(message)).  hit == false: ask the software verifier.
func (p *Provider) MemoLookup(qx, qy *[32]byte, signature, digest []byte) (status uint8, hit bool) {
	if len(signature) == 0 || len(digest) == 0 || atomic.LoadUint32(&p.poisoned) != 0 {
		return 0, false
	}
	var st C.uint8_t
	rc := C.fabgpu_csp_memo_lookup(p.csp, (*C.uint8_t)(unsafe.Pointer(&qx[0])), (*C.uint8_t)(unsafe.Pointer(&qy[0])),
		(*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)), (*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &st)
	return uint8(st), rc == 0
}

// MemoLookupNym is MemoLookup for an idemix pseudonym signature: the entry is bound to the issuer key the caller verifies under
// (issuerHash = idemix.IssuerPublicKey.Hash of bccsp.IdemixNymSignerOpts.IssuerPK) - two channels may define one idemix MSP id with
// different issuer keys, and provider and memo are shared by all channels.
func (p *Provider) MemoLookupNym(issuerHash, nymX, nymY *[32]byte, signature, digest []byte) (status uint8, hit bool) {
	if len(signature) == 0 || len(digest) == 0 || atomic.LoadUint32(&p.poisoned) != 0 {
		return 0, false
	}
	var st C.uint8_t
	rc := C.fabgpu_csp_memo_lookup_nym(p.csp, (*C.uint8_t)(unsafe.Pointer(&issuerHash[0])), (*C.uint8_t)(unsafe.Pointer(&nymX[0])),
		(*C.uint8_t)(unsafe.Pointer(&nymY[0])), (*C.uint8_t)(unsafe.Pointer(&signature[0])), C.size_t(len(signature)),
		(*C.uint8_t)(unsafe.Pointer(&digest[0])), C.size_t(len(digest)), &st)
	return uint8(st), rc == 0
}

// HasBlock: are memo entries seeded under blockSeq still there?  (extensions/gossip/state pre-verifies a block when it ARRIVES;
// the validator wrapper asks this before it would marshal and submit the block a second time.)
func (p *Provider) HasBlock(blockSeq uint64) bool {
	if running, ok := p.inflight.Load(blockSeq); ok {
		<-running.(chan struct{}) // a pass under this name is in flight: its verdicts are a few hundred microseconds away
	}
	if atomic.LoadUint32(&p.poisoned) != 0 {
		return false
	}
	var n C.uint64_t
	return C.fabgpu_csp_memo_has_block(p.csp, C.uint64_t(blockSeq), &n) == 0 && n > 0
}

// RegisterIdemixMSP makes the block pass verify the pseudonym signatures of creators serialized under mspID
// (RegisterIdemixMSPsOfConfig, idemix_config.go, calls this for every idemix MSP of a channel's committed configuration with the
// marshalled idemix.IssuerPublicKey its msp/idemixmsp.go:99-173 Setup imports).
// The pass sees MSP ids, not channels: a channel's latest key for an MSP id replaces its earlier one (a config update that rotates the
// issuer key), and while two channels' current keys for one MSP id differ that MSP id's creators stay with bccsp/idemix.
// false: not accelerated (a key the device does not take, or one whose Hash field is not the hash of the rest of the key - the
// reference recomputes it, idemix/issuerkey.go:171-182, and so does the library).
func (p *Provider) RegisterIdemixMSP(channelID, mspID string, ipkBytes []byte) bool {
	if len(ipkBytes) == 0 {
		return false
	}
	cc := C.CString(channelID)
	defer C.free(unsafe.Pointer(cc))
	cs := C.CString(mspID)
	defer C.free(unsafe.Pointer(cs))
	var id C.int64_t
	rc := C.fabgpu_csp_idemix_msp_register2(p.csp, cc, cs, (*C.uint8_t)(unsafe.Pointer(&ipkBytes[0])), C.size_t(len(ipkBytes)), &id)
	return rc == 0 && id >= 0
}

// SetMSPHashFamily tells the block pass the hash family of an MSP: family is the MSP config's
// CryptoConfig.SignatureHashFamily ("SHA2", "SHA3"; msp/mspimplsetup.go:81-101 reads it, identity.getHashOpt uses it).  The P-384
// creators and endorsers of an MSP set "SHA3" are then hashed with SHA3-256 by the pass (options P384 and SHA3 both on); every MSP is
// SHA2 until set.  A change holds for the passes that start after the call.  The error is getHashOpt's for an unknown family, and says
// that bccsp/sw serves SHA3 while the SHA3 option is off: the MSP's signatures are then decided by bccsp/sw, as before.
func (p *Provider) SetMSPHashFamily(mspID, family string) error {
	cm := C.CString(mspID)
	defer C.free(unsafe.Pointer(cm))
	cf := C.CString(family)
	defer C.free(unsafe.Pointer(cf))
	text := make([]byte, 256)
	rc := C.fabgpu_csp_msp_hash_family(p.csp, cm, cf, (*C.char)(unsafe.Pointer(&text[0])), C.size_t(len(text)))
	if rc == 0 {
		return nil
	}
	if rc < 0 {
		return errors.Errorf("fabgpu_csp_msp_hash_family: %s", C.GoString(C.fabgpu_strerror(rc)))
	}
	n := 0
	for n < len(text) && text[n] != 0 {
		n++
	}
	return errors.New(string(text[:n]))
}

// PassRoutes: how the block passes of this provider went - walked on the device (DESIGN 4.4b) or on the host - and why the last
// block was declined by the device walk (not staged, idemix MSPs registered, a certificate beyond the device decoder).  For metrics.
func (p *Provider) PassRoutes() (deviceWalks, hostWalks uint64, lastDecline string) {
	var d, h C.uint64_t
	why := make([]byte, 256)
	C.fabgpu_csp_pass_routes(p.csp, &d, &h, (*C.char)(unsafe.Pointer(&why[0])), C.size_t(len(why)))
	n := 0
	for n < len(why) && why[n] != 0 {
		n++
	}
	return uint64(d), uint64(h), string(why[:n])
}

// MemoStats is for metrics / tests.
func (p *Provider) MemoStats() (entries, hits, misses, evicted uint64) {
	var e, h, m, v C.uint64_t
	C.fabgpu_csp_memo_stats(p.csp, &e, &h, &m, &v)
	return uint64(e), uint64(h), uint64(m), uint64(v)
}

// MemoStatsP384: the same counters of the verdict memo of the pass's P-384 tuples (Options.P384; a table of its own: MemoStats does not
// count its entries or lookups).
func (p *Provider) MemoStatsP384() (entries, hits, misses, evicted uint64) {
	var e, h, m, v C.uint64_t
	C.fabgpu_csp_memo_stats_p384(p.csp, &e, &h, &m, &v)
	return uint64(e), uint64(h), uint64(m), uint64(v)
}

// ---- metrics (SURVEY.md section 5: next to gossip_privdata_validation_duration, gossip/metrics/metrics.go:161-187) ----

var (
	passDurationOpts = metrics.HistogramOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "block_pass_duration",
		Help: "Time it takes to pre-verify every signature of a block on the GPU (in seconds): marshalled block in, verdict memo seeded",
	}
	passTxOpts = metrics.CounterOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "block_pass_transactions",
		Help: "Transactions that went through the block pre-verify pass",
	}
	passSigOpts = metrics.CounterOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "block_pass_signatures",
		Help: "Creator, endorsement and orderer signatures the block pre-verify pass derived from blocks",
	}
	passFailedOpts = metrics.CounterOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "block_pass_failures",
		Help: "Block pre-verify passes that ended in an infrastructure error (validation then ran on bccsp/sw)",
	}
	passRouteOpts = metrics.GaugeOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "block_passes",
		Help: "Block pre-verify passes by route: walked on the device, walked on the host, and per device context",
		LabelNames: []string{"route"}, StatsdFormat: "%{#fqname}.%{route}",
	}
	memoOpts = metrics.GaugeOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "verdict_memo",
		Help: "Verdict memo: entries held, bccsp.Verify lookups answered (hits), lookups left to bccsp/sw (misses), entries evicted; digest memo: bccsp.Hash calls answered (hash_hits) / left to bccsp/sw (hash_misses), block copies held, copies refused",
		LabelNames: []string{"what"}, StatsdFormat: "%{#fqname}.%{what}",
	}
	memoP384Opts = metrics.GaugeOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "verdict_memo_p384",
		Help: "Verdict memo of the block pass's P-384 tuples (Options.P384): entries held, bccsp.Verify lookups for P-384 keys answered (hits), lookups left to the coalesced entry or bccsp/sw (misses), entries evicted",
		LabelNames: []string{"what"}, StatsdFormat: "%{#fqname}.%{what}",
	}
	auditMismatchOpts = metrics.CounterOpts{
		Namespace: "fabgpu", Name: "audit_mismatches",
		Help: "Results of the device that the provider's sampled CPU audit re-computed and found different (the first one poisons the provider)",
	}
	auditNymOpts = metrics.GaugeOpts{
		Namespace: "fabgpu", Name: "audit_pseudonyms",
		Help: "Idemix pseudonym results and the provider's sampled CPU audit: verified again on the CPU (audited), sampled but not auditable because the block copy or the issuer's fields were not held (skipped)",
		LabelNames: []string{"what"}, StatsdFormat: "%{#fqname}.%{what}",
	}
	keyTablesOpts = metrics.GaugeOpts{
		Namespace: "bccsp", Subsystem: "gpu", Name: "key_tables",
		Help: "Comb tables of registered P-256 keys on the first device context: keys live, slots draining behind a retirement, keys retired for evicted identities, registrations that reused a retired slot, slots parked for good, bytes of device memory held",
		LabelNames: []string{"what"}, StatsdFormat: "%{#fqname}.%{what}",
	}
	poisonedOpts = metrics.GaugeOpts{
		Namespace: "fabgpu", Name: "poisoned",
		Help: "1 once the GPU provider has retired itself after a CPU audit mismatch and serves everything from bccsp/sw, else 0",
	}
)

type passMetrics struct {
	duration         metrics.Histogram
	tx, sigs, failed metrics.Counter
	routes, memo     metrics.Gauge
	memoP384         metrics.Gauge
	auditMismatches  metrics.Counter
	auditNym         metrics.Gauge
	poisoned         metrics.Gauge
	keyTables        metrics.Gauge
}

func (m *passMetrics) passDone(d time.Duration, nTx, nSig, seeded int) {
	if m == nil {
		return
	}
	m.duration.Observe(d.Seconds())
	m.tx.Add(float64(nTx))
	m.sigs.Add(float64(nSig))
}

func (m *passMetrics) passFailed() {
	if m != nil {
		m.failed.Add(1)
	}
}

// RegisterMetrics wires the provider's counters into the peer's metrics provider.  Call once where the peer creates its other
// metrics (internal/peer/node/start.go:243: metricsProvider := opsSystem.Provider - the patch line is in gpufactory_patch.txt); the
// route and memo gauges are refreshed every refresh interval from the library's own counters (PassRoutes, PassesPerDevice, MemoStats).
func (p *Provider) RegisterMetrics(mp metrics.Provider, refresh time.Duration) {
	if mp == nil {
		return
	}
	p.metricsOnce.Do(func() {
		m := &passMetrics{
			duration: mp.NewHistogram(passDurationOpts), tx: mp.NewCounter(passTxOpts), sigs: mp.NewCounter(passSigOpts),
			failed: mp.NewCounter(passFailedOpts), routes: mp.NewGauge(passRouteOpts), memo: mp.NewGauge(memoOpts),
			auditMismatches: mp.NewCounter(auditMismatchOpts), poisoned: mp.NewGauge(poisonedOpts),
			auditNym: mp.NewGauge(auditNymOpts),
			memoP384: mp.NewGauge(memoP384Opts),
			keyTables: mp.NewGauge(keyTablesOpts),
		}
		m.poisoned.Set(0)
		if refresh <= 0 {
			refresh = 5 * time.Second
		}
		p.stopMetrics = make(chan struct{})
		p.metricsDone = make(chan struct{})
		p.mv.Store(m)
		go func() {
			defer close(p.metricsDone)
			t := time.NewTicker(refresh)
			defer t.Stop()
			var mismatchesSeen uint64
			for {
				select {
				case <-p.stopMetrics:
					return
				case <-t.C:
				}
				d, h, _ := p.PassRoutes()
				m.routes.With("route", "device_walk").Set(float64(d))
				m.routes.With("route", "host_walk").Set(float64(h))
				for i, n := range p.PassesPerDevice() {
					m.routes.With("route", "context_"+strconv.Itoa(i)).Set(float64(n))
				}
				e, hit, miss, ev := p.MemoStats()
				m.memo.With("what", "entries").Set(float64(e))
				m.memo.With("what", "hits").Set(float64(hit))
				m.memo.With("what", "misses").Set(float64(miss))
				m.memo.With("what", "evicted").Set(float64(ev))
				if p.p384 {
					e, hit, miss, ev = p.MemoStatsP384()
					m.memoP384.With("what", "entries").Set(float64(e))
					m.memoP384.With("what", "hits").Set(float64(hit))
					m.memoP384.With("what", "misses").Set(float64(miss))
					m.memoP384.With("what", "evicted").Set(float64(ev))
				}
				hh, hm, hb, _, hr := p.HashMemoStats()
				m.memo.With("what", "hash_hits").Set(float64(hh))
				m.memo.With("what", "hash_misses").Set(float64(hm))
				m.memo.With("what", "hash_blocks_held").Set(float64(hb))
				m.memo.With("what", "hash_copies_refused").Set(float64(hr))
				kl, kd, kr, kp, kb, kret := p.KeyTableStats(0)
				m.keyTables.With("what", "live").Set(float64(kl))
				m.keyTables.With("what", "draining").Set(float64(kd))
				m.keyTables.With("what", "retired").Set(float64(kret))
				m.keyTables.With("what", "reused").Set(float64(kr))
				m.keyTables.With("what", "parked").Set(float64(kp))
				m.keyTables.With("what", "bytes_held").Set(float64(kb))
				if _, _, _, mm, _, _ := p.AuditStats(); mm > mismatchesSeen {
					m.auditMismatches.Add(float64(mm - mismatchesSeen))
					mismatchesSeen = mm
				}
				na, ns := p.NymAuditStats()
				m.auditNym.With("what", "audited").Set(float64(na))
				m.auditNym.With("what", "skipped").Set(float64(ns))
				if p.Poisoned() { // (a lookup that met the mismatch only answers "miss": this is where the Go side learns of it)
					m.poisoned.Set(1)
				}
			}
		}()
	})
}
