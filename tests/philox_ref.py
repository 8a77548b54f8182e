"""TEST INFRASTRUCTURE: the one Python copy of the device noise of include/mdx.h (mdx_latent_renoise_*, mdx_cfg_ddim_eta_step_*).

A numpy Philox4x32-10 (tests/test_latent_renoise_contract.py holds it to the Random123 known answers) and the documented mapping
words -> normals in float64.  Counter word 3 is the stream's domain: 0 = a jump of ops.LatentRenoise (noise_ref), 1 = a step of
ops.DdimEtaStep (eta_noise_ref).  Imported by the contract tests, the kernel tests, tests/op_parity.py and tests/plan_interp.py: the two
whole-plan instruments share this function and nothing else."""
import numpy as np

DOMAIN_JUMP, DOMAIN_STEP = 0, 1


def philox4x32_10(ctr, key):
    """Philox4x32-10 on uint32 arrays: ctr [..., 4], key [..., 2] -> [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
        k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
    return np.stack(c, -1).astype(np.uint32)


def words(seed, counter, count, first_block=0, domain=DOMAIN_JUMP):
    """The uint32 words [ceil(count / 4), 4] of one group from block first_block on: counter (lo32(k), hi32(k), counter, domain),
    key (lo32(seed), hi32(seed))."""
    k = np.arange(first_block, first_block + (count + 3) // 4, dtype=np.uint64)
    ctr = np.stack([k & 0xFFFFFFFF, k >> 32, np.full_like(k, int(counter) & 0xFFFFFFFF), np.full_like(k, domain)], -1)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(ctr, np.broadcast_to(np.array([s & 0xFFFFFFFF, s >> 32], dtype=np.uint64), (len(k), 2)))


def normals(w, count):
    """float64 z of `count` consecutive elements from the words [blocks, 4], by the mapping of include/mdx.h."""
    u1 = lambda x: ((x >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = lambda x: (x >> 8).astype(np.float64) * 2.0 ** -24
    z = np.empty((len(w), 4))
    for a in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u1(w[:, a])))
        z[:, a], z[:, a + 1] = rad * np.cos(2 * np.pi * u2(w[:, a + 1])), rad * np.sin(2 * np.pi * u2(w[:, a + 1]))
    return z.reshape(-1)[:count]


def noise_words(seed, visit, count, first_block=0):
    """A jump's words: counter (lo32(k), hi32(k), visit, 0)."""
    return words(seed, visit, count, first_block, DOMAIN_JUMP)


def noise_ref(seed, visit, count, first_block=0):
    """float64 z of `count` consecutive elements of one group of a jump, starting at relative index 4 * first_block."""
    return normals(noise_words(seed, visit, count, first_block), count)


def eta_noise_words(seed, draw, count, first_block=0):
    """A stochastic step's words: counter (lo32(k), hi32(k), draw, 1)."""
    return words(seed, draw, count, first_block, DOMAIN_STEP)


def eta_noise_ref(seed, draw, count, first_block=0):
    """float64 z of `count` consecutive elements of one group of a stochastic step (renoise's mapping, counter word 3 = 1)."""
    return normals(eta_noise_words(seed, draw, count, first_block), count)


def shared_blocks(wa, wb):
    """How many 4-word blocks two word tables have in common."""
    rows = lambda w: set(map(bytes, np.ascontiguousarray(w)))
    return len(rows(wa) & rows(wb))
