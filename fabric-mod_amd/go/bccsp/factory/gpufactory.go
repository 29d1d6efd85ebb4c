// +build fabgpu

// GPUFactory: the bccsp/factory side of ProviderName "GPU" (pattern: bccsp/factory/pkcs11factory.go:17-45).
// Drop into the reference tree as bccsp/factory/gpufactory.go and apply the two `case`s of gpufactory_patch.txt to
// nopkcs11.go / pkcs11.go (initFactories and GetBCCSPFromOpts switch on the provider name; there is no runtime BCCSP plugin
// loader in this version - SURVEY.md 8(b) "Selection").  core.yaml:  peer.BCCSP.Default: GPU  (+ the usual SW section, which
// configures the embedded software provider: hash family, security level, key store).
// NOT compiled in this repository (no Go toolchain in the build image); Go 1.14 compatible.
package factory

import (
	"github.com/hyperledger/fabric/bccsp"
	"github.com/hyperledger/fabric/bccsp/gpu"
	"github.com/pkg/errors"
)

const (
	// GPUBasedFactoryName is the name of the factory of the MI355X-accelerated BCCSP implementation
	GPUBasedFactoryName = "GPU"
)

// GPUOpts is the `GPU:` section of the BCCSP configuration.
type GPUOpts struct {
	// Devices: the HIP ordinals this node's ONE provider drives, one device context each (an ordinal may repeat: several contexts on
	// one GPU).  Empty = every visible device.  factory.GetDefault() is process-global (bccsp/factory/factory.go:41-55) and every
	// channel's validator receives it (core/peer/peer.go:337-355), so "one provider per device" cannot be configured - one provider
	// owns them all and routes each block pass to the least busy device (fabgpu_csp_new2, include/fabgpu_bccsp.h).
	Devices []int `mapstructure:"devices" json:"devices" yaml:"Devices"`
	// Device: DEPRECATED alias from the time a provider drove one device (`GPU: Device: N`).  mapstructure ignores unknown keys, so
	// without this field an old core.yaml would silently mean "every visible device" - contexts and ConcurrentPasses' pinned memory
	// on all of them.  Used only when Devices is empty: Devices = [Device].  Setting both to different things is an error.
	Device *int `mapstructure:"device" json:"device,omitempty" yaml:"Device,omitempty"`
	// ConcurrentPasses: per device, how many overlapping block passes to allocate for when the provider is made (staging slots, pinned
	// memo tables, pass arrays) instead of when passes first overlap.  2 suits the arrival pipeline of one channel per device.
	ConcurrentPasses int `mapstructure:"concurrentpasses" json:"concurrentpasses" yaml:"ConcurrentPasses"`
	// ExpectBlockBytes / ExpectTuples size that pre-allocation; 0 = 64 MiB / 65 536 signatures (configtx.yaml AbsoluteMaxBytes and
	// MaxMessageCount x (1 + endorsements) are the numbers to put here).
	ExpectBlockBytes int `mapstructure:"expectblockbytes" json:"expectblockbytes" yaml:"ExpectBlockBytes"`
	ExpectTuples     int `mapstructure:"expecttuples" json:"expecttuples" yaml:"ExpectTuples"`
	// MemoBlocks: how many pre-verified blocks the verdict memo may hold while they wait for their validators - MemoBlocks x ExpectTuples
	// entries.  The bounded memo drops its OLDEST block first, which during a state transfer is the one the committer needs next, so this
	// must not be smaller than what the payload buffer accepts ahead: peer.gossip.state.blockBufferSize (core.yaml, default 20; the
	// arrival hook only pre-verifies blocks the buffer kept).  0 = the library's 2^18 entries (six 10 000-transaction blocks).
	MemoBlocks int `mapstructure:"memoblocks" json:"memoblocks" yaml:"MemoBlocks"`
	// NoHashMemo switches the digest memo off: bccsp.Hash always goes to bccsp/sw and no pass keeps a host copy of its block.  By default a
	// pass keeps its block in pinned host memory of the library until the block is evicted (HashMemoBlocks copies per device at a time;
	// 0: MemoBlocks + ConcurrentPasses, at least 8 - each as large as its block), and identity.Verify's Hash (msp/identities.go:173-181)
	// is answered from it when the validator's bytes equal the block's, byte for byte.
	NoHashMemo     bool `mapstructure:"nohashmemo" json:"nohashmemo" yaml:"NoHashMemo"`
	HashMemoBlocks int  `mapstructure:"hashmemoblocks" json:"hashmemoblocks" yaml:"HashMemoBlocks"`
	// KeyTables16: every public key the provider imports (the endorsers' and creators' keys of the channels' MSPs - msp/cache/cache.go:14-18
	// keeps a hundred identities) also gets a 16-bit comb table on the device: 80 MiB each, built behind the import, the first 64 keys.
	// Launches whose keys all have one verify with 16 mixed additions for u2*Q instead of 32: registered-key verification 170 -> 214-231 M/s
	// on an MI355X; 5 GiB of its 288 GB.
	KeyTables16 bool `mapstructure:"keytables16" json:"keytables16" yaml:"KeyTables16"`
	// HostWalk keeps the envelope walk of the block pass on the host (A/B runs); PassTiming prints every pass's stage breakdown.
	HostWalk   bool `mapstructure:"hostwalk" json:"hostwalk" yaml:"HostWalk"`
	PassTiming bool `mapstructure:"passtiming" json:"passtiming" yaml:"PassTiming"`
	// CoalesceVerify: Verify calls that miss the verdict memo share device launches with whatever other misses are in flight
	// (fabgpu_csp_verify_coalesced).  For the orderer (General.BCCSP in orderer.yaml): its Broadcast handlers reach
	// identity.Verify one message per goroutine behind SigFilter and no block pass precedes them.  Leave it off on peers.
	CoalesceVerify bool `mapstructure:"coalesceverify" json:"coalesceverify" yaml:"CoalesceVerify"`
	// AuditPermille: the share (0 .. 1000) of the digests and verdicts the provider is about to hand out from the device that it
	// re-computes on the CPU first; the first disagreement poisons the provider for good and everything is served by bccsp/sw from then
	// on (gpu.go Provider.Poisoned; metrics fabgpu_audit_mismatches, fabgpu_poisoned).  Unset means 1 - one hit in a thousand, about
	// thirty verdicts and thirty digests of a 10 000-transaction block; `AuditPermille: 0` switches the audit off, 1000 audits everything.
	AuditPermille *int `mapstructure:"auditpermille" json:"auditpermille,omitempty" yaml:"AuditPermille,omitempty"`
	// RetireEvictedKeys: an identity that the provider's identity cache evicts also gives up its comb table on every device
	// (fabgpu_bccsp.h option "retire_evicted_keys"), so a peer whose clients come and go keeps registering the keys that are hot now;
	// without it a context stops registering after 4096 keys and serves every later identity on the fresh-key kernels until the
	// peer restarts.  Unset means true; `RetireEvictedKeys: false` keeps every table registered for the life of the process.
	RetireEvictedKeys *bool `mapstructure:"retireevictedkeys" json:"retireevictedkeys,omitempty" yaml:"RetireEvictedKeys,omitempty"`
	// SHA3: identities of an MSP whose SignatureHashFamily is SHA3 (msp/identities.go:216-224) are verified in batches on the device too
	// (fabgpu_bccsp.h option "hash_sha3").  Unset means true; `SHA3: false` leaves the family to bccsp/sw.  The block pass hashes with
	// SHA-256 either way: a SHA3 MSP's signatures are decided by bccsp/sw behind it.
	SHA3 *bool `mapstructure:"sha3" json:"sha3,omitempty" yaml:"SHA3,omitempty"`
	// P384: Verify on an ECDSA P-384 key asks the device first (fabgpu_bccsp.h option "p384", fabgpu_csp_verify_coalesced_p384) and takes
	// only "valid" from it.  Default false: P-384 keys stay with bccsp/sw.  The block pass leaves P-384 endorsers to bccsp/sw either way.
	P384 bool `mapstructure:"p384" json:"p384,omitempty" yaml:"P384,omitempty"`
	// P384Wide: registered P-384 keys are verified with eight lanes per signature in launches of at most 8 192 rows (fabgpu.h
	// FABGPU_FLAG_P384_WIDE, fabgpu_bccsp.h option "p384_wide").  Default false.  Verdicts do not depend on it; it needs P384.
	P384Wide bool `mapstructure:"p384wide" json:"p384wide,omitempty" yaml:"P384Wide,omitempty"`
	// P384KeyTables16: every imported P-384 key also gets a 16-bit comb table on the device, 144 MiB each and at most 32 per context
	// (fabgpu.h FABGPU_FLAG_P384_KEY_TABLES_16BIT, fabgpu_bccsp.h option "p384_key_tables16").  Default false.  Verdicts do not depend
	// on it; it needs P384.
	P384KeyTables16 bool `mapstructure:"p384keytables16" json:"p384keytables16,omitempty" yaml:"P384KeyTables16,omitempty"`
	// SHA3Coop: SHA3-256 launches of at most 4 096 messages run with 32 lanes on a message, and larger launches hash their few long
	// messages that way (fabgpu.h FABGPU_FLAG_SHA3_COOP, fabgpu_bccsp.h option "sha3_coop").  Default false.  Digests and verdicts do
	// not depend on it; it matters only where SHA3 is served.
	SHA3Coop bool `mapstructure:"sha3coop" json:"sha3coop,omitempty" yaml:"SHA3Coop,omitempty"`
}

// DefaultAuditPermille is what GPUOpts.AuditPermille means when the `GPU:` section does not set it.
const DefaultAuditPermille = 1

// GPUFactory is the factory of the GPU-accelerated BCCSP.
type GPUFactory struct{}

// Name returns the name of this factory
func (f *GPUFactory) Name() string {
	return GPUBasedFactoryName
}

// Get returns an instance of BCCSP using Opts: the software provider built from SwOpts exactly as SWFactory builds it,
// wrapped by the GPU provider.  If no usable device exists the error is returned: a peer configured for "GPU" should not
// silently run without one (operators who want the fallback configure "SW").
func (f *GPUFactory) Get(config *FactoryOpts) (bccsp.BCCSP, error) {
	if config == nil || config.SwOpts == nil {
		return nil, errors.New("Invalid config. It must not be nil.")
	}
	swCSP, err := (&SWFactory{}).Get(config)
	if err != nil {
		return nil, errors.Wrapf(err, "Failed initializing the software BCCSP behind the GPU provider")
	}
	opts := gpu.Options{AuditPermille: DefaultAuditPermille, RetireEvictedKeys: true, SHA3: true}
	if g := config.GPUOpts; g != nil {
		if g.Device != nil {
			if len(g.Devices) == 0 {
				g.Devices = []int{*g.Device}
			} else if len(g.Devices) != 1 || g.Devices[0] != *g.Device {
				return nil, errors.Errorf("Invalid GPU opts: the deprecated Device [%d] contradicts Devices %v", *g.Device, g.Devices)
			}
		}
		opts = gpu.Options{Devices: g.Devices, ConcurrentPasses: g.ConcurrentPasses, ExpectBlockBytes: g.ExpectBlockBytes,
			ExpectTuples: g.ExpectTuples, MemoBlocks: g.MemoBlocks, HostWalk: g.HostWalk, PassTiming: g.PassTiming,
			NoHashMemo: g.NoHashMemo, HashMemoBlocks: g.HashMemoBlocks, KeyTables16: g.KeyTables16, AuditPermille: DefaultAuditPermille, RetireEvictedKeys: true, SHA3: true}
		opts.P384 = g.P384
		opts.P384Wide = g.P384Wide
		opts.P384KeyTables16 = g.P384KeyTables16
		opts.SHA3Coop = g.SHA3Coop
		if g.SHA3 != nil {
			opts.SHA3 = *g.SHA3
		}
		if g.RetireEvictedKeys != nil {
			opts.RetireEvictedKeys = *g.RetireEvictedKeys
		}
		if g.AuditPermille != nil {
			if *g.AuditPermille < 0 || *g.AuditPermille > 1000 {
				return nil, errors.Errorf("Invalid GPU opts: AuditPermille [%d] must be 0 .. 1000", *g.AuditPermille)
			}
			opts.AuditPermille = *g.AuditPermille
		}
	}
	csp, err := gpu.New(swCSP, opts)
	if err != nil {
		return nil, err
	}
	if config.GPUOpts != nil && config.GPUOpts.CoalesceVerify {
		if p, ok := csp.(*gpu.Provider); ok {
			p.SetCoalesce(true)
		}
	}
	return csp, nil
}
