// The witness solver's square-root rows (polymath_amd/host/solve_plan.hpp: sqrt_row, KIND_SQRT; polymath_amd/csrc/sqrt.cuh: fr_sqrt;
// polymath_amd/csrc/divrem.cuh: marker_byte) on the CPU.  The accepted shapes against hand-written plans; byte 4 anywhere else (an
// ordinary row, beside a second unknown, a rest beside u, u in C_r, a bit of a decomposition, a pair's flag, a quotient's position),
// where it is what the plain marker is; marker_byte on the four markers and their near-misses; fr_sqrt on edge operands against
// literals computed with Python integers; a corpus (a level of 40 square roots, the decompression of three Edwards points, a system
// that mixes a square root with a division and an is-zero pair) on which build_plan_any_order equals build_plan field by field in
// matrix order and which, reversed and under seeded permutations, plans with every column at its in-order level and EXECUTES --
// serially, with the host field type and the routines the kernels call -- to the in-order assignment; the same corpus with the plain
// marker, which is refused with the words it always had; a square-root row that waits for its C side; and a non-residue, stuck at its
// own row and reported as the root cause under a reordered plan.
// Built and run by tests/test_native_solve_sqrt.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include <array>

#include "solve_selftest.hpp"

struct RootLiteral {
    uint64_t c[4], root[4];   // canonical integers; a root of all ones: c is a non-residue
};
// {c, the smaller root of c}: 0, 1, 4, r - 1, the generator (a non-residue), then for j = 0 .. s  c = y^2 with y = ROOT^(2^(s - j)) h,
// ROOT = g^((r - 1) / 2^s) and h = 3^(2^s) of odd order: y's 2-power part has order 2^j, which drives every iteration of the loop nest
static const RootLiteral BLS_ROOTS[] = {
    {{0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x0000000000000004ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000002ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0xffffffff00000000ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}, {0x0001000000000000ull, 0xec03000276030000ull, 0x8d51ccce760304d0ull, 0x0000000000000000ull}},
    {{0x0000000000000007ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0xffffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffffull}},
    {{0x10cacbbe1bac3bfbull, 0x645f73609acfe531ull, 0x85b92420f0e01d00ull, 0x5f4b3b3cd34e11d0ull}, {0xadbf0bfa7d45a980ull, 0x9d5b566e8177b278ull, 0x21d1231c1f3add65ull, 0x04f99923c421b2d4ull}},
    {{0x10cacbbe1bac3bfbull, 0x645f73609acfe531ull, 0x85b92420f0e01d00ull, 0x5f4b3b3cd34e11d0ull}, {0xadbf0bfa7d45a980ull, 0x9d5b566e8177b278ull, 0x21d1231c1f3add65ull, 0x04f99923c421b2d4ull}},
    {{0xef353440e453c406ull, 0xef5e30a2652e76cdull, 0xad80b3e718c1bb04ull, 0x14a26c16564f6b77ull}, {0x5f7c3e33be04d2d6ull, 0x430a706fa9e50b6eull, 0xc56a5bade07bb02full, 0x3017caed3c035d0eull}},
    {{0xf95ac8da61abd0f7ull, 0xa2e2c42fdef50e32ull, 0xfdfc5940e39b80e1ull, 0x672c05e59a2e1254ull}, {0xacf83f054267d126ull, 0x2218fa8654b54304ull, 0xe4b60c47c6edd70bull, 0x394687f5f6a57cdfull}},
    {{0xc86352d97c73d43dull, 0xdb0d34c08bd82f70ull, 0xfe16d172260ff38aull, 0x6c1a855fa18e3849ull}, {0xd38114827dbf9274ull, 0x00f531b5777f4eecull, 0x71de5e2d271e17f6ull, 0x1bf170d6f104088bull}},
    {{0x014bdbe3d96d05b2ull, 0xa29c05a557f4d5b4ull, 0xbba1677f02b9817dull, 0x376a03409d5aaec4ull}, {0xd66dc9e87a79a1c0ull, 0x18b20b1e5d00d3f1ull, 0xe145da8d36b0546dull, 0x2358b8136da319efull}},
    {{0x7986f28606c5d953ull, 0x07c8442ba5a794d2ull, 0xb05d49ee6430b60cull, 0x42ab8ab629e19fa3ull}, {0x2975613b639c3c04ull, 0x7fe4449d26f0384bull, 0x738ddcfcba9e69fcull, 0x34d5cd0a5030f21cull}},
    {{0x862b03bfd068ecc2ull, 0xf536e16a5e38e641ull, 0x62655b88853e837dull, 0x25fedad40182a47dull}, {0xfcf7a74ab81a17baull, 0x5408ed760774127aull, 0x8c6b6af796cbedffull, 0x1b0a153d9ec522e3ull}},
    {{0xaad95bea5396cab6ull, 0x24f6fe0a4d318b72ull, 0x4906b20f2b52414aull, 0x6bb8985f35ae1919ull}, {0x5ae534d8721d5eb2ull, 0x315f30a290e95d09ull, 0x94b526f0aef62a5eull, 0x334d8c9d5b154beaull}},
    {{0xeac8490bdb616c77ull, 0x736872b136494ccdull, 0x3c9cd9f7b0407d3eull, 0x55ce286e120312c2ull}, {0xba660b45807698a1ull, 0x815203bd9a45843cull, 0x3c3bfc6911e4ac9bull, 0x2b4555ac0f36c04full}},
    {{0x8a8617bb12735fa8ull, 0xd0e613e2bce5bc03ull, 0xb54971db843a112cull, 0x08a85ddbda9140c6ull}, {0x596efbc9229ab9f4ull, 0xc47abce0b780ccceull, 0x3596213f00cdb1b6ull, 0x289eb998925cdc06ull}},
    {{0xa8b94543b521316cull, 0xc72a5f4051d22b7cull, 0x652c3a30f7392fceull, 0x10fea805951c918aull}, {0x2d196c6fc233498bull, 0x229decaac5a4a638ull, 0x41cad6d0604530baull, 0x1af2320ce1fbaf78ull}},
    {{0xd4b3b4370d823defull, 0x20aedf7062718505ull, 0x71302a18824e88adull, 0x5bd0b9b9969d4f3dull}, {0xe1367fdfa63aea4dull, 0xf75b23ce48d980afull, 0xbd118db486a4689dull, 0x33412e5d5e52f01eull}},
    {{0x36b02b8b9a96b1cfull, 0x3576bf6a15805cacull, 0x383a0b05509b4df0ull, 0x678398372b3b2c67ull}, {0xb662d38b96d7a52aull, 0x5f228b7cc773139eull, 0x021f82a2abea129eull, 0x1a11fc1b65390435ull}},
    {{0x63697af1fa275276ull, 0x4c3dbec97a29f148ull, 0xaece830de46054f7ull, 0x7006e4a97949d4acull}, {0x40a163b306da2f5aull, 0x602f117a43ce8fd3ull, 0x4246cef29b8c93ccull, 0x144549335e329705ull}},
    {{0xeb3f6301f0c16602ull, 0xcb5add9c34daf37dull, 0x65e9791e67cd376eull, 0x5d26125ac66e0567ull}, {0xeff1fcda9b5acb60ull, 0x430b0cf2cdf8b230ull, 0x8a39e6cea8ee2aa2ull, 0x2dba14a5a9ed34acull}},
    {{0x3def8071e8a66bceull, 0x9eb4b75b1332acdaull, 0x1f29e10299edd384ull, 0x157bae896d8628e8ull}, {0x0be4937a582d9949ull, 0x15aae1add8725383ull, 0xdf80be700befc843ull, 0x1ff4ddec5049fccbull}},
    {{0x6c4f56e3971bf0b3ull, 0x7d00b15442fa7cd2ull, 0xbc181206df6f396bull, 0x30b7c8fe3fa345f9ull}, {0x1ad7d166b68f316eull, 0x052685ae8762ff8full, 0x72ff6074c25c2055ull, 0x371b6611f6546d25ull}},
    {{0x669d46f13f8e2e69ull, 0x7b8da9cf2b90f0ebull, 0xfcb2a61586848bf8ull, 0x3fbbd5a0411027abull}, {0x6ce868fca431fe5bull, 0x366d1ae7e08d571full, 0x19381c22707af534ull, 0x09417ac6b7e0ff81ull}},
    {{0x5b42e9a43e1b5829ull, 0x353fbbc23a3032dcull, 0x2def066280a9c27full, 0x679624cf8155d2ecull}, {0x1c8683d3fb2996e0ull, 0x054560c4919505c0ull, 0xf0da5baf3861eaebull, 0x09b07c3a4c062db7ull}},
    {{0xed3dd4c766227289ull, 0x8ce1acbc74acddfcull, 0xda60b976669e29a6ull, 0x7003a7f758a61fc9ull}, {0x72ed4b8ae2961f0eull, 0xf55c254e87b16b62ull, 0x90261b0fd36b3189ull, 0x3689ae6039c2f744ull}},
    {{0x4aefcae79162552full, 0x4efade3a786851a3ull, 0x79703f3462d97473ull, 0x1625701074935a75ull}, {0x2e657f2c72fe7ed4ull, 0x91d7a01cc93180c3ull, 0x4a1b04bd5c0a8ee0ull, 0x0a51e90f74bc18b0ull}},
    {{0xee0a795f0936d562ull, 0xc691ba31bb331cbfull, 0x5d2ad99d4762709dull, 0x050a75a93592c3fbull}, {0x5bd630ad06536773ull, 0x964f66dc9c68a91eull, 0xbfaac1edbd585ae5ull, 0x0e6ee668f87bb200ull}},
    {{0xae1278c99991dad7ull, 0x76acb86a887f9696ull, 0xf14a09c13fb4adf6ull, 0x713072a0a39d895dull}, {0x6cd1e854dfad26dfull, 0x64625c4211be67f3ull, 0xbf126423a8821503ull, 0x30cd093cadceb18dull}},
    {{0xf7c9bf6006b99efeull, 0xa586fc1326b5cf30ull, 0x6f0c676495c9fd5cull, 0x4642120b1b9ff339ull}, {0x2eea72d809e36fd8ull, 0x6c1c592d95cce32dull, 0x8739dc558c452c33ull, 0x3274262f1fe590adull}},
    {{0x907410434535813bull, 0xb9716202b0a17b6eull, 0x4e6282483167bb81ull, 0x2800d2c88760c5e7ull}, {0x75ca2cd9d54976bbull, 0xbc86fb9400ca3810ull, 0x07b05967eef1e411ull, 0x1c3908b528764d67ull}},
    {{0x9d1c7c77c6c365f0ull, 0xcbd36281122c718cull, 0xa66122becf01c7c3ull, 0x6f21b022a956cc00ull}, {0xf55509efb1b91fbcull, 0xa14bc7ab354ebccbull, 0xf6ac5108f73fce32ull, 0x35d4758328e94253ull}},
    {{0x565a35e7b26fbb7eull, 0x481ddcd980619c72ull, 0xfeaef08765ae689eull, 0x5f10c51e030b4290ull}, {0xd44548cb41909ebdull, 0x52fda4a3bd17ecc2ull, 0x2bead0e1a8080262ull, 0x0b356f4d3047857bull}},
    {{0x8212ded213f8f3a1ull, 0x9c942f9dbd885dabull, 0xef8fc07d138fb591ull, 0x31902e11ac7ee11bull}, {0x03b459a5db34a5e9ull, 0x98b930244441d4b7ull, 0x9903b7c398ac0225ull, 0x0ad6eb4f967cf648ull}},
    {{0x890a6697c3cc548cull, 0x33d00356764cedfbull, 0x91d8ed0431e2bad2ull, 0x42a1ca578375339full}, {0x2085b1254e13e505ull, 0xa5a7a47d42672fc3ull, 0x45364821f07ca602ull, 0x2740eb5f5dbee4d1ull}},
    {{0x045c1d461d5736dcull, 0x0e8b7d9ef111d6c9ull, 0xf8549330789cd016ull, 0x46ce380fab088df8ull}, {0x0323c110ab721c53ull, 0x08af545ddb1b1d83ull, 0x152376ed1cbcc6ddull, 0x2920b6a457308b99ull}},
    {{0xc1e2472cf9927cd9ull, 0x75dfa7d7af75665bull, 0xb1361c86899408faull, 0x3ed1a28ae034a646ull}, {0xa834b6a69e1af0f0ull, 0xb47fc8a116a237c2ull, 0xb11cdaed9f8ff5e6ull, 0x06828f8fdf716e8aull}},
    {{0xf7b0053400f7d76cull, 0x5f97585b02067526ull, 0x457875c8a3459b78ull, 0x2f2e4e9b4e661aafull}, {0x1d6641f41e11b20full, 0x9585ed5687e6a946ull, 0x9d6b3ee14e858aecull, 0x04e12e0276335422ull}},
};
static const RootLiteral BN_ROOTS[] = {
    {{0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x0000000000000004ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0x0000000000000002ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x43e1f593f0000000ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, {0x20cff123608fc9cbull, 0xcb49c3517c4604a5ull, 0xb3c4d79d41a91758ull, 0x0000000000000000ull}},
    {{0x0000000000000005ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}, {0xffffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffffull}},
    {{0xef8db3d0662258a5ull, 0x0e227a941686d5d4ull, 0x3602854379b198d0ull, 0x0c778771401bdf60ull}, {0x991fcbe1710fdf0dull, 0x1e5f70f15ca8d985ull, 0x6fe377e077e9d33full, 0x03dab7ef4c0658a7ull}},
    {{0xef8db3d0662258a5ull, 0x0e227a941686d5d4ull, 0x3602854379b198d0ull, 0x0c778771401bdf60ull}, {0x991fcbe1710fdf0dull, 0x1e5f70f15ca8d985ull, 0x6fe377e077e9d33full, 0x03dab7ef4c0658a7ull}},
    {{0x545441c389dda75cull, 0x1a116db463329abcull, 0x824dc07307cfbf8dull, 0x23ecc701a115c0c9ull}, {0x7fd06d87330e4df0ull, 0xbbdf28b99d0bf1a3ull, 0x610cc4a7ce821091ull, 0x01b7dbc03d6265a5ull}},
    {{0xc1ecbeb7913634a2ull, 0x2048f441ae4aa9ecull, 0x0c381b087add4db1ull, 0x04a40d0bc9a8a8e6ull}, {0x7580bbbdaa623593ull, 0x3c52d60b35e1a433ull, 0x97695086448f9b30ull, 0x0dfba5c90e5fa46full}},
    {{0xbe93199d56422876ull, 0xa07c1ce93d557456ull, 0x5271f800e1074883ull, 0x0a6f5ae0cec94e55ull}, {0xccb1de86323a0277ull, 0xd50316a32b260698ull, 0x37ce96978937f244ull, 0x0703a8d8feec954cull}},
    {{0x54be5c1cdfed6c53ull, 0x925fa7affb9962b0ull, 0xa89c1f8148fc6c65ull, 0x10ae4e7cd05729efull}, {0xad9ce461d5cfe60bull, 0xfa76a7c63c1d6418ull, 0x963e2890f6c3b03bull, 0x0d400bd1637b0de0ull}},
    {{0x1396df6eee75b609ull, 0xbc54f6f6b5b90410ull, 0xfb39057502835ed6ull, 0x159417fef6adda3eull}, {0xd05b0e63ddaaddc5ull, 0x46ba06e016148bc3ull, 0x43282355d4d7bf73ull, 0x15a6841b944b4c41ull}},
    {{0x1204e0aedcfc9b21ull, 0xcc71cc414974648aull, 0xc1b0fc378ff8cebeull, 0x28a3935e0894a20aull}, {0x12d858dcc146f12eull, 0x28b67ee2dd1ac97eull, 0xe22683cef69a1e81ull, 0x0392e0f1e158aab8ull}},
    {{0x698bd360ed652b16ull, 0x992656a820745477ull, 0xa1621fccbc646524ull, 0x2a93311da7ad808aull}, {0x1ca02be879d51ed7ull, 0xbc89074003b2b291ull, 0xbd9e60b9e09f9e4dull, 0x17e4f0b080724561ull}},
    {{0x5a5bcefe5deca86aull, 0x93ae81ae193b024cull, 0xeaad7e026334f719ull, 0x0372287e13b5bba3ull}, {0x83ce140f92e9e7dbull, 0x42af0f2fa19f5440ull, 0x7811fabe08d34e14ull, 0x04c7c432c8d7e8dcull}},
    {{0x6f48348004644c02ull, 0x33e4faf7a4d94c9dull, 0x8bc36495c56fbb2dull, 0x25a949e8b63459c2ull}, {0x4b73c175a22c32b8ull, 0x6b5eadbf1a6d960eull, 0xa237d7aa71a10a0eull, 0x0bf322d5cfa4860eull}},
    {{0x5e6174dc4b70168bull, 0xadd9c3bd902ae379ull, 0x307e42e2e979cc57ull, 0x1f33332d2810b3bbull}, {0x85cc809280657442ull, 0x885accf90a055a70ull, 0x9685e72a36ee7569ull, 0x172850236eedfd28ull}},
    {{0xd44972241d2c353aull, 0x7d562cb08165b65cull, 0xd665e0733cd95888ull, 0x019f77614a7a77fdull}, {0x8c8633b86cd1eb76ull, 0x66bf96d58e0793b6ull, 0xd0ace655469e2119ull, 0x17814d926015968dull}},
    {{0x3ab60dffe6730a52ull, 0x71b414ebdaf95807ull, 0x9e65c716ea528025ull, 0x0e033219dd7c7b24ull}, {0xb19a4287c479edf5ull, 0xc881110c0691db82ull, 0x89ac59de8cd67a8cull, 0x01f392db41c44f3eull}},
    {{0x9a1f3b08186f86b4ull, 0x592dffce6df343a5ull, 0x9bd0286a239d4d82ull, 0x29a60f5ec3ffa0ddull}, {0x44694e7296a38fffull, 0xc3b88777722929d1ull, 0xdd834155485f030full, 0x0abcb66514914173ull}},
    {{0xad17fca4f158beb0ull, 0xe8c59f8c7cd7f1f5ull, 0x18db776fe93ed11bull, 0x23ec305d2b2b7219ull}, {0x1f8987a83e8325f1ull, 0x3da008b56adfb138ull, 0x674b44d8af7729bbull, 0x0a98a06abd06f3ddull}},
    {{0x7f2d9955e4ec8416ull, 0x08cf4a1c364e8222ull, 0x8989cbaad7dd7e34ull, 0x1d4345510de714ebull}, {0x342f595389a3a7c0ull, 0x20985d393eeb8e78ull, 0x3b07e2aa1eeb5d74ull, 0x0f9656572d7d2071ull}},
    {{0x3d9c8f17551cd337ull, 0x078a5e99849a059eull, 0x5090451f3aab1430ull, 0x04177c547926dba4ull}, {0xe7c0ef1bb84bc6f3ull, 0x48263e391097f453ull, 0x7e976195dd8935a6ull, 0x094e52b9cf165021ull}},
    {{0xad52c8d10800ed4eull, 0xf3685d2d3b29095dull, 0x58e9e87f38ac6ab7ull, 0x11c3b43d059c293eull}, {0xec1fe85321fc9730ull, 0xee9812b0b7706012ull, 0xcf2f86c3451d4aceull, 0x10781d3c6ff58639ull}},
    {{0xe42d829c8aa98c5eull, 0xb1035daf08b8e9a3ull, 0xf4c4086974503e31ull, 0x13e359e5a952bc62ull}, {0xc6b0e04a6399e8a4ull, 0x8f5fc71abc4abf58ull, 0x16aca192d0d59516ull, 0x0163af3331857b11ull}},
    {{0x30b87a01fbd3cb20ull, 0xa62023f2485f01bdull, 0xd6bf7cfda4bc17a3ull, 0x251f2288adb97f37ull}, {0x3856cff4604e1586ull, 0xba865819672cb220ull, 0x7730c5f7f15e9d25ull, 0x0957c36d37fee069ull}},
    {{0x5e431586ce4439a1ull, 0x7aaec6449c0eadc7ull, 0x0896df8dd34e2d1dull, 0x15236973f020d30full}, {0xcf75078c2d2f8929ull, 0xfaa8ceecff7e876bull, 0x7c34fc9677ef2e9cull, 0x02de0895487ab665ull}},
    {{0x0307989e5784f76eull, 0xd04bdc90431bdf9cull, 0x2b8465031cd43a40ull, 0x14631cf4027bdacdull}, {0xd3a96d292a71337eull, 0x165b1ed8d1072f9dull, 0xfc265117b5ab62a6ull, 0x137fac9d50398009ull}},
    {{0x184635b373bc3255ull, 0xf1ec141f04548141ull, 0xd57d861aecb3f0e4ull, 0x0a719352d251f3aeull}, {0xbfbcf3ea3c15b18eull, 0xf7de51da3be02ed4ull, 0x24daa252ba0470b6ull, 0x0275cadf3c778108ull}},
    {{0x6afeb5be44e51920ull, 0x5ad9a651fc54e0adull, 0x1fc7bcf234990695ull, 0x06b465865dd73426ull}, {0x3dc7590220b4582cull, 0xc5412030721311f5ull, 0x748cf0e80232a310ull, 0x0bcb2c85624bedbdull}},
    {{0xf46d6e397f185a9eull, 0x9d9cdc03cba2aaa7ull, 0x837f269e274e3bbbull, 0x12511f06d96eeed0ull}, {0xb08e1fb001c308e8ull, 0x2284a5e2a7081ee9ull, 0xda6eea34f7018ba1ull, 0x14def700b0e447cbull}},
    {{0x16371e6b5e28c215ull, 0xab1ce3ebd23d7a42ull, 0xeab9e7e0594fe594ull, 0x0adabae757b020b5ull}, {0x451e3bbea8a25bb8ull, 0x96b7366794bd2119ull, 0xdc7f248a17e7034full, 0x0d6bb2223b7828bcull}},
    {{0xf9fdde53ffa42a63ull, 0x2779984a7a23f219ull, 0xf69e5fafeac1d464ull, 0x0c14fce8d9844fdbull}, {0x39ef6d920f0f644eull, 0x66797e2e7df5fd68ull, 0xd59b2d2d41cac51eull, 0x06dd9e534d3273a1ull}},
    {{0x13425f3ff1f11f62ull, 0xeb27a544ff0ed5b9ull, 0x291f9cdc67d88ca5ull, 0x160f64eec77fef02ull}, {0x04461041c6784b2full, 0x947869d8b32e651full, 0x03e44fcf8e35bbbeull, 0x128266ea0426fbceull}},
};
// Jubjub's d = -(10240 / 10241) mod r; Baby Jubjub's a and d are small
static const uint64_t JUBJUB_D[4] = {0x01065fd6d6343eb1ull, 0x292d7f6d37579d26ull, 0xf5fd9207e6bd7fd4ull, 0x2a9318e74bfa2b48ull};

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit Suite(const char *n) : Rig(n) {}

    static Fr sqrt_marker() { Fr m = marker(); m.l[6] = 0xfffffffeu; return m; }      // bit 192: the lowest bit of the top 64-bit word
    static Fr from_words(const uint64_t w[4]) {
        Fr v;
        memcpy(v.l, w, 32);
        return pm::to_mont<P>(v);
    }
    // pattern bytes: 1 on `cols`, 2 on `quotients`, 3 on `indicators`, 4 on `roots`
    static std::vector<uint8_t> pattern(const System &s, const std::vector<uint32_t> &cols, const std::vector<uint32_t> &roots, const std::vector<uint32_t> &quotients = {},
                                        const std::vector<uint32_t> &indicators = {}) {
        std::vector<uint8_t> un = s.unknown(cols, quotients, indicators);
        for (uint32_t j : roots) un[j] = PATTERN_SQRT;
        return un;
    }
    // the canonical integer of v is <= (r - 1) / 2
    bool is_small(const Fr &v) const {
        const Fr c = pm::from_mont<P>(v);
        uint64_t w[4], half[4];
        memcpy(w, c.l, 32);
        for (int i = 0; i < 4; ++i) half[i] = modulus[i] >> 1 | (i < 3 ? modulus[i + 1] << 63 : 0);
        return !words_less(half, w);
    }
    // Euler's criterion, a^((r - 1) / 2) == 1, by square-and-multiply on the modulus' words: independent of fr_sqrt
    bool is_residue(const Fr &a) const {
        Fr acc = F::one();
        for (int bit = 255; bit >= 1; --bit) {      // the bits of (r - 1) / 2 = r >> 1
            acc = F::mul(acc, acc);
            if ((modulus[bit >> 6] >> (bit & 63)) & 1) acc = F::mul(acc, a);
        }
        return acc.eq(F::one());
    }

    // ---- 1. the accepted shapes, against plans written by hand.  0 one | 1 s, 2 t given | 3 u
    //   (ka u) * (kb u) = C  with ka, kb in {1, 7, -1}; C empty, a constant or a combination of the two signals; a stored zero
    //   coefficient in front of u in A_r, or in B_r
    void shapes() {
        const Fr one = F::one(), m1 = F::neg(one);
        const Fr ks[3] = {one, u(7), m1};
        static const char *const CSIDE[3] = {"empty", "a constant", "two signals"};
        static const char *const ZEROS[3] = {"no stored zero", "a stored zero before u in A", "a stored zero before u in B"};
        for (int ia = 0; ia < 3; ++ia)
            for (int ib = 0; ib < 3; ++ib)
                for (int cside = 0; cside < 3; ++cside)
                    for (int zeros = 0; zeros < 3; ++zeros) {
                        const std::string tag = std::string("shapes: ka ") + std::to_string(ia) + ", kb " + std::to_string(ib) + ", C " + CSIDE[cside] + ", " + ZEROS[zeros];
                        const Fr kk = F::mul(ks[ia], ks[ib]), c25 = F::mul(kk, u(25));      // C z = ka kb 5^2
                        const Fr s_v = rnd(), t_v = F::sub(c25, F::mul(u(3), s_v));         // 3 s + t = ka kb 25
                        System s; s.mw = 3;
                        Row a = {{ks[ia], 3}}, b = {{ks[ib], 3}}, c;
                        if (zeros == 1) a.insert(a.begin(), std::pair<Fr, uint32_t>(F::zero(), 1));
                        if (zeros == 2) b.insert(b.begin(), std::pair<Fr, uint32_t>(F::zero(), 2));
                        if (cside == 1) c = {{c25, 0}};
                        if (cside == 2) c = {{u(3), 1}, {one, 2}};
                        s.add(a, b, c);
                        const std::vector<uint8_t> unknown = pattern(s, {}, {3});
                        for (uint32_t wide : {WIDE_STEPS, 1u}) {
                            const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                            bool ok = p.error == OK && p.message.empty() && p.steps.size() == 1 && p.divs.empty() && p.pairs.empty() && p.bit_cols.empty() && !p.reordered;
                            if (ok) {
                                Step want{zeros == 1 ? 1u : 0u, 0, 3, KIND_SQRT, 1};
                                want.cols_off = zeros == 2 ? 1 : 0;
                                ok = same_step(p.steps[0], want) && p.level_ptr == std::vector<uint32_t>({0, 1}) && p.launches.size() == 1 &&
                                     same_launch(p.launches[0], wide == 1 ? Launch{0, 1, LAUNCH_SQRT, 1} : Launch{0, 1, LAUNCH_CHAIN, 1}) && well_sorted(p);
                            }
                            check(ok, tag + ": the plan is the hand-written one, and its launch divides");
                            check(same_plan(p, q) && q.launches.size() == p.launches.size() && (q.launches.empty() || (q.launches[0].kind == LAUNCH_SQRT) == (p.launches[0].kind == LAUNCH_SQRT)),
                                  tag + ": the any-order builder gives the same plan");
                            if (!ok) continue;
                            std::vector<Fr> z = {one, s_v, t_v, sqrt_marker()};
                            const Fr want_root = cside == 0 ? F::zero() : u(5);
                            check(execute(s, p, z) == NONE && z[3].eq(want_root) && rows_hold(s, z), tag + ": executes to the smaller root");
                        }
                        const Plan bare = in_order(s, unknown, WIDE_STEPS, false);
                        check(bare.error == ERR_TWO_MATRICES && bare.steps.empty(), tag + ": without the modulus the rule is off");
                    }
        // a non-residue on the C side: stuck at the row, zero stored
        System s; s.mw = 3;
        s.add(Row{{one, 3}}, Row{{one, 3}}, Row{{one, 1}});
        const Plan p = in_order(s, pattern(s, {}, {3}));
        std::vector<Fr> z = {one, u(C::ID == 0 ? 7 : 5), u(0), sqrt_marker()};
        check(p.error == OK && execute(s, p, z) == 0 && z[3].is_zero(), "shapes: the generator is a non-residue: stuck at row 0, zero stored");
    }

    // ---- 2. byte 4 has meaning in the square-root row only: every plan is the plain marker's
    void marker_elsewhere() {
        const Fr one = F::one(), m1 = F::neg(one);
        struct Other { const char *what; uint64_t mw; std::vector<std::array<Row, 3>> rows; std::vector<uint32_t> plain; uint32_t col; int error; };
        const Row lc = {{one, 1}, {m1, 2}};
        const std::vector<Other> others = {
            // 0 one | 1 a, 2 b given | 3 u
            {"an ordinary row: u named once", 3, {{Row{{one, 3}}, Row{{one, 1}}, Row{{one, 2}}}}, {}, 3, OK},
            {"an ordinary row: u in C", 3, {{Row{{one, 1}}, Row{{one, 2}}, Row{{u(7), 3}}}}, {}, 3, OK},
            {"a rest beside u: (u + a)(u + a) = b", 3, {{Row{{one, 3}, {one, 1}}, Row{{one, 3}, {one, 1}}, Row{{one, 2}}}}, {}, 3, ERR_TWO_MATRICES},
            {"a rest beside u on one side only", 3, {{Row{{one, 3}}, Row{{one, 3}, {one, 1}}, Row{{one, 2}}}}, {}, 3, ERR_TWO_MATRICES},
            {"u in C_r: u u = u + b", 3, {{Row{{one, 3}}, Row{{one, 3}}, Row{{one, 3}, {one, 2}}}}, {}, 3, ERR_TWO_MATRICES},
            // 0 one | 1 a, 2 b given | 3 u, 4 v
            {"beside a second unknown: u (a + v) = 0", 4, {{Row{{one, 3}}, Row{{one, 1}, {one, 4}}, Row{}}}, {4}, 3, ERR_MANY_UNKNOWNS},
            {"beside a second unknown in C_r: u u = v", 4, {{Row{{one, 3}}, Row{{one, 3}}, Row{{one, 4}}}}, {4}, 3, ERR_MANY_UNKNOWNS},
            // 0 one | 1 a, 2 b given | 3 flag, 4 m: ark's pair
            {"a pair's flag", 4, {{lc, Row{{one, 4}}, Row{{one, 3}}}, {lc, Row{{one, 0}, {m1, 3}}, Row{}}}, {4}, 3, OK},
            {"a pair's multiplier", 4, {{lc, Row{{one, 4}}, Row{{one, 3}}}, {lc, Row{{one, 0}, {m1, 3}}, Row{}}}, {3}, 4, OK},
            // 0 one | 1 a, 2 b given | 3 q, 4 rem: q * b = a - rem with byte 4 where the quotient's marker belongs -- the opener's shape, never closed
            {"a quotient's position", 4, {{Row{{one, 3}}, Row{{one, 2}}, Row{{one, 1}, {m1, 4}}}}, {4}, 3, ERR_MANY_UNKNOWNS},
        };
        for (const Other &o : others) {
            System s; s.mw = o.mw;
            for (const auto &r : o.rows) s.add(r[0], r[1], r[2]);
            std::vector<uint32_t> all = o.plain;
            all.push_back(o.col);
            const Plan p = in_order(s, pattern(s, o.plain, {o.col})), plain = in_order(s, pattern(s, all, {}));
            const Plan q = any_order(s, pattern(s, o.plain, {o.col})), plain_q = any_order(s, pattern(s, all, {}));
            check(p.error == o.error && count_kind(p, KIND_SQRT) == 0 && same_plan(p, plain), std::string("marker elsewhere: ") + o.what + ": the plan of the plain marker, word for word");
            check(count_kind(q, KIND_SQRT) == 0 && same_plan(q, plain_q), std::string("marker elsewhere: ") + o.what + ": ... and in any order");
        }
        {   // the ordinary row executes: u * 2 = 8.  0 one | 1 a, 2 b given | 3 u
            System s; s.mw = 3;
            s.add(Row{{one, 3}}, Row{{one, 1}}, Row{{one, 2}});
            const Plan p = in_order(s, pattern(s, {}, {3}));
            std::vector<Fr> z = {one, u(2), u(8), sqrt_marker()};
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_A && execute(s, p, z) == NONE && z[3].eq(u(4)) && rows_hold(s, z), "marker elsewhere: u * 2 = 8 executes as the ordinary row it is");
        }
        {   // bits with byte 4: a decomposition as before, and the kernels' marker test passes over all four markers.  1 x given | 2 .. 5 bits
            System s; s.mw = 5;
            s.boolean(2); s.boolean(3); s.boolean(4); s.boolean(5);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}, {u(4), 4}, {u(8), 5}});
            const Plan p = in_order(s, pattern(s, {2}, {5}, {3}, {4}));
            std::vector<Fr> z = {one, u(14), marker(), Rig::quotient_marker(), Rig::indicator_marker(), sqrt_marker()};
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_BITS_C && same_plan(p, in_order(s, pattern(s, {2, 3, 4, 5}, {}))) && execute(s, p, z) == NONE &&
                      z[2].is_zero() && z[3].eq(one) && z[4].eq(one) && z[5].eq(one),
                  "marker elsewhere: a byte-4 column as a bit of a decomposition");
        }
        {   // boolean-pending first, then its square-root row: that row is the square-root step.  1 c given | 2 u
            System s; s.mw = 2;
            s.boolean(2);
            s.add(Row{{one, 2}}, Row{{one, 2}}, Row{{one, 1}});
            const Plan p = in_order(s, pattern(s, {}, {2}));
            std::vector<Fr> z = {one, one, sqrt_marker()};
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_SQRT && p.steps[0].row == 1 && execute(s, p, z) == NONE && z[2].eq(one),
                  "marker elsewhere: a boolean-pending byte-4 column is taken by its square-root row");
        }
    }

    // ---- 3. marker_byte, and one pattern per batch on the BYTES (solve.hip: k_solve_pattern).  0 one | 1 c | 2 u, 3 v
    void markers() {
        const Fr one = F::one();
        check(pm::marker_byte<P>(marker()) == 1 && pm::marker_byte<P>(Rig::quotient_marker()) == 2 && pm::marker_byte<P>(Rig::indicator_marker()) == 3 &&
                  pm::marker_byte<P>(sqrt_marker()) == 4,
              "markers: the four markers give 1, 2, 3 and 4");
        // the near-misses that were: bits 0 and 64 both clear, bit 65 clear, bit 128 clear, the top bit clear (on each marker), ...fffffffc
        Fr both = Rig::quotient_marker(), near3 = marker(), other = marker(), near = marker();
        both.l[2] = 0xfffffffeu;
        near3.l[2] = 0xfffffffcu;
        other.l[4] = 0xfffffffeu;
        near.l[0] = 0xfffffffcu;
        bool none = pm::marker_byte<P>(both) == 0 && pm::marker_byte<P>(near3) == 0 && pm::marker_byte<P>(other) == 0 && pm::marker_byte<P>(near) == 0 &&
                    pm::marker_byte<P>(F::zero()) == 0 && pm::marker_byte<P>(F::neg(one)) == 0;
        for (Fr top : {marker(), Rig::quotient_marker(), Rig::indicator_marker(), sqrt_marker()}) {
            top.l[7] = 0x7fffffffu;
            none = none && pm::marker_byte<P>(top) == 0;
        }
        check(none, "markers: the near-misses that were are no markers");
        // the new ones: bit 192 clear together with bit 0, together with bit 64, and bit 193 clear
        Fr with0 = sqrt_marker(), with64 = sqrt_marker(), bit193 = marker(), both193 = sqrt_marker();
        with0.l[0] = 0xfffffffeu;
        with64.l[2] = 0xfffffffeu;
        bit193.l[6] = 0xfffffffdu;
        both193.l[6] = 0xfffffffcu;
        check(pm::marker_byte<P>(with0) == 0 && pm::marker_byte<P>(with64) == 0 && pm::marker_byte<P>(bit193) == 0 && pm::marker_byte<P>(both193) == 0,
              "markers: bit 192 clear with bit 0 or bit 64 clear, and bit 193 clear, are no markers");
        uint32_t limbs[8];
        uint64_t words[4];
        memcpy(limbs, sqrt_marker().l, sizeof limbs);
        memcpy(words, limbs, sizeof words);
        check(pm::marker_byte_limbs(limbs) == 4 && words[0] == ~(uint64_t)0 && words[1] == ~(uint64_t)0 && words[2] == ~(uint64_t)0 && words[3] == ~(uint64_t)1 &&
                  !words_less(words, modulus),
              "markers: the routine on limbs; the marker is 2^256 - 1 - 2^192 and >= r");
        const std::vector<Fr> first = {one, u(4), sqrt_marker(), sqrt_marker()}, second = {one, u(9), sqrt_marker(), marker()};
        std::vector<uint8_t> bytes(4);
        uint64_t mismatch = NONE;
        for (uint64_t j = 0; j < 4; ++j) {
            bytes[j] = pm::marker_byte<P>(first[j]);
            if (pm::marker_byte<P>(second[j]) != bytes[j] && ((uint64_t)1 << 32 | j) < mismatch) mismatch = (uint64_t)1 << 32 | j;
        }
        check(bytes == std::vector<uint8_t>({0, 0, PATTERN_SQRT, PATTERN_SQRT}), "markers: the bytes of assignment 0");
        check(mismatch == ((uint64_t)1 << 32 | 3), "markers: assignment 1 differs from assignment 0 at column 3");
    }

    // ---- 4. fr_sqrt on the edge operands, against the literals
    void roots() {
        const RootLiteral *lits = C::ID == 0 ? BLS_ROOTS : BN_ROOTS;
        const size_t n = C::ID == 0 ? sizeof BLS_ROOTS / sizeof *BLS_ROOTS : sizeof BN_ROOTS / sizeof *BN_ROOTS;
        check(n == 5 + (size_t)C::TWO_ADICITY + 1, "roots: 0, 1, 4, r - 1, the generator and one operand per j = 0 .. s");
        for (size_t i = 0; i < n; ++i) {
            const Fr c = from_words(lits[i].c);
            const bool residue = ~(lits[i].root[0] & lits[i].root[1] & lits[i].root[2] & lits[i].root[3]) != 0;
            Fr root = marker();
            const bool ok = pm::fr_sqrt<P>(c, &root);
            check(ok == residue && is_residue(c) == (residue && !c.is_zero()), "roots: literal " + std::to_string(i) + ": a residue or not, as Euler's criterion says");
            if (residue) check(ok && root.eq(from_words(lits[i].root)) && is_small(root) && F::mul(root, root).eq(c), "roots: literal " + std::to_string(i) + ": the smaller root");
            else check(root.eq(marker()), "roots: literal " + std::to_string(i) + ": nothing is written for a non-residue");
        }
        for (int i = 0; i < 16; ++i) {      // both roots' squares give the same small root
            const Fr y = rnd(), c = F::mul(y, y), c2 = F::mul(F::neg(y), F::neg(y));
            Fr r1 = F::zero(), r2 = F::zero();
            const bool ok = pm::fr_sqrt<P>(c, &r1) && pm::fr_sqrt<P>(c2, &r2);
            check(ok && r1.eq(r2) && is_small(r1) && (r1.eq(y) || r1.eq(F::neg(y))), "roots: y^2 and (-y)^2 give the one small root, which is y or -y");
        }
    }

    // ---- 5. the corpus
    struct Case {
        std::string what;
        System s;
        std::vector<uint32_t> unknown, quotients, roots;
        std::vector<std::vector<uint32_t>> groups;      // rows that keep their relative order under every permutation (a pair's rows)
        uint32_t first_root_row = 0;                    // with plain markers the matrix order is refused at this row ...
        uint32_t first_root_col = 0;                    // ... naming this column
        int rounds = 1;
        std::function<std::vector<Fr>(int)> given;      // round -> z with the given columns set, markers elsewhere
    };
    Case square_roots() {   // 0 one | 1 out | per i: 2 + 2 i c_i given, 3 + 2 i u_i:  u_i * u_i = c_i;  (sum u_i) * 1 = out
        Case c; c.what = "square roots";
        const uint32_t width = 40;
        c.s.m0 = 2; c.s.mw = 2 * width;
        Row sum;
        for (uint32_t i = 0; i < width; ++i) {
            c.s.add(Row{{F::one(), 3 + 2 * i}}, Row{{F::one(), 3 + 2 * i}}, Row{{F::one(), 2 + 2 * i}});
            c.roots.push_back(3 + 2 * i);
            sum.push_back({F::one(), 3 + 2 * i});
        }
        c.s.add(sum, Row{{F::one(), 0}}, Row{{F::one(), 1}});
        c.unknown = {1};
        c.first_root_row = 0; c.first_root_col = 3;
        const size_t ncols = c.s.m0 + c.s.mw;
        const std::vector<uint32_t> roots = c.roots;
        std::vector<Fr> ys;
        for (uint32_t i = 0; i < 2 * width; ++i) ys.push_back(rnd());
        c.rounds = 2;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one();
            for (uint32_t i = 0; i < width; ++i) z[2 + 2 * i] = i == 7 ? F::zero() : F::mul(ys[round * width + i], ys[round * width + i]);
            for (uint32_t j : roots) z[j] = sqrt_marker();
            return z;
        };
        return c;
    }
    // 0 one | 1 out | per point, from `base`: y, sign given, y2, u, x0, x, then nb bits of x0
    //   y y = y2;  (a - d y2) u = 1 - y2;  x0 x0 = u;  sign (1 - sign) = 0;  x0 (1 - 2 sign) = x;  booleanity rows;  x0 * 1 = sum 2^i b_i;  (sum x) * 1 = out
    Case decompress() {
        Case c; c.what = "decompress";
        const Fr one = F::one(), m1 = F::neg(one);
        const Fr a = C::ID == 0 ? m1 : u(168700), d = C::ID == 0 ? from_words(JUBJUB_D) : u(168696);
        const uint32_t points = 3, nb = bit_length(modulus) - 1, per = 6 + nb;
        c.s.m0 = 2; c.s.mw = points * per;
        Row sum;
        for (uint32_t pt = 0; pt < points; ++pt) {
            const uint32_t y = 2 + pt * per, sign = y + 1, y2 = y + 2, uu = y + 3, x0 = y + 4, x = y + 5, bits = y + 6;
            c.s.add(Row{{one, y}}, Row{{one, y}}, Row{{one, y2}});
            c.s.add(Row{{a, 0}, {F::neg(d), y2}}, Row{{one, uu}}, Row{{one, 0}, {m1, y2}});
            if (pt == 0) c.first_root_row = (uint32_t)c.s.nr();
            c.s.add(Row{{one, x0}}, Row{{one, x0}}, Row{{one, uu}});
            c.s.add(Row{{one, sign}}, Row{{one, 0}, {m1, sign}}, Row{});
            c.s.add(Row{{one, x0}}, Row{{one, 0}, {F::neg(u(2)), sign}}, Row{{one, x}});
            Row weighted;
            Fr weight = one;
            for (uint32_t i = 0; i < nb; ++i) {
                c.s.boolean(bits + i);
                weighted.push_back({weight, bits + i});
                weight = F::add(weight, weight);
                c.unknown.push_back(bits + i);
            }
            c.s.add(Row{{one, x0}}, Row{{one, 0}}, weighted);
            c.roots.push_back(x0);
            for (uint32_t j : {y2, uu, x}) c.unknown.push_back(j);
            sum.push_back({one, x});
        }
        c.s.add(sum, Row{{one, 0}}, Row{{one, 1}});
        c.unknown.push_back(1);
        c.first_root_col = 2 + 4;
        // ordinates of curve points: the first y = 2, 3, ... for which (1 - y^2) / (a - d y^2) is a square, by Euler's criterion
        std::vector<Fr> ys;
        for (uint64_t y = 2; ys.size() < 2 * points; ++y) {
            const Fr y2 = F::mul(u(y), u(y)), den = F::sub(a, F::mul(d, y2));
            if (!den.is_zero() && is_residue(F::mul(F::sub(one, y2), F::inv(den)))) ys.push_back(u(y));
        }
        const size_t ncols = c.s.m0 + c.s.mw;
        const std::vector<uint32_t> roots = c.roots;
        c.rounds = 2;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = one;
            for (uint32_t pt = 0; pt < points; ++pt) {
                z[2 + pt * per] = ys[round * points + pt];
                z[3 + pt * per] = (pt + round) % 2 ? one : F::zero();
            }
            for (uint32_t j : roots) z[j] = sqrt_marker();
            return z;
        };
        return c;
    }
    // 0 one | 1 out | 2 c, 3 a given | 4 u | 5 q, 6 rem | 7 flag, 8 m
    //   u u = c;  q * u = a - rem;  ark's pair on rem;  (q + flag + u) * 1 = out
    Case mixed() {
        Case c; c.what = "mixed";
        c.s.m0 = 2; c.s.mw = 7;
        const Fr one = F::one(), m1 = F::neg(one);
        c.s.add(Row{{one, 4}}, Row{{one, 4}}, Row{{one, 2}});
        c.s.add(Row{{one, 5}}, Row{{one, 4}}, Row{{one, 3}, {m1, 6}});
        const uint32_t b = c.s.boolean(7);
        c.s.add(Row{{one, 6}}, Row{{one, 8}}, Row{{one, 7}});
        c.s.add(Row{{one, 6}}, Row{{one, 0}, {m1, 7}}, Row{});
        c.groups.push_back({b, b + 1, b + 2});
        c.s.add(Row{{one, 5}, {one, 7}, {one, 4}}, Row{{one, 0}}, Row{{one, 1}});
        c.unknown = {1, 6, 7, 8};
        c.quotients = {5};
        c.roots = {4};
        c.first_root_row = 0; c.first_root_col = 4;
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;      // rem != 0 and rem == 0
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[2] = u(121); z[3] = u(round ? 22 : 23); z[4] = sqrt_marker(); z[5] = Rig::quotient_marker();
            return z;
        };
        return c;
    }
    void corpus() {
        std::vector<Case> cases;
        cases.push_back(square_roots());
        cases.push_back(decompress());
        cases.push_back(mixed());
        for (Case &c : cases) {
            System &s = c.s;
            const std::vector<uint8_t> unknown = pattern(s, c.unknown, c.roots, c.quotients);
            for (uint32_t wide : {WIDE_STEPS, 2u}) {
                const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                bool ok = p.error == OK && count_kind(p, KIND_SQRT) == c.roots.size() && p.divs.size() == c.quotients.size() && well_sorted(p);
                for (const Launch &l : p.launches)
                    for (uint32_t t = l.lo; ok && t < l.hi; ++t) ok = l.kind == LAUNCH_CHAIN ? (p.steps[t].kind != KIND_SQRT || l.divides) : (p.steps[t].kind == KIND_SQRT) == (l.kind == LAUNCH_SQRT);
                check(ok, c.what + ": plans in order; a wide launch holds square-root rows only or none, and a launch with one divides");
                bool same = same_plan(p, q) && !q.reordered;
                for (size_t t = 0; same && t < p.launches.size(); ++t) same = (p.launches[t].kind == LAUNCH_SQRT) == (q.launches[t].kind == LAUNCH_SQRT);
                check(same, c.what + ": in order the any-order builder is build_plan, field by field");
            }
            const Plan p = in_order(s, unknown);
            if (p.error != OK) continue;
            if (c.what == "square roots")
                check(p.launches.size() == 2 && same_launch(p.launches[0], Launch{0, 40, LAUNCH_SQRT, 1}) && same_launch(p.launches[1], Launch{40, 41, LAUNCH_CHAIN, 0}) &&
                          p.levels() == 2,
                      "square roots: one square-root launch of its own, which divides, then the sum, which does not");
            if (c.what == "decompress")
                check(p.levels() == 5 && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_CHAIN && p.launches[0].divides && count_kind(p, KIND_BITS_C) == 3 && count_kind(p, KIND_B) == 3,
                      "decompress: five levels in one dividing chain: y2, u, x0, x and the bits, the sum");
            if (c.what == "mixed")
                check(p.levels() == 4 && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_CHAIN && p.launches[0].divides && p.pairs.size() == 1 && p.steps[0].kind == KIND_SQRT,
                      "mixed: one dividing chain: the root, the division by it, the pair, the sum");
            const std::vector<uint32_t> levels = column_levels(s, p);
            std::vector<std::vector<Fr>> want;
            for (int round = 0; round < c.rounds; ++round) {
                std::vector<Fr> z = c.given(round);
                bool ok = execute(s, p, z) == NONE && rows_hold(s, z);
                for (const Fr &v : z) ok = ok && !is_marker(v);
                for (uint32_t j : c.roots) ok = ok && is_small(z[j]);
                check(ok, c.what + ": the in-order plan executes to an assignment that satisfies the rows, every root the smaller one");
                want.push_back(z);
            }
            if (c.what == "square roots") check(want[0][3 + 2 * 7].is_zero(), "square roots: the root of zero is zero");
            if (c.what == "decompress") check(want[0][2 + 5].eq(want[0][2 + 4]) && want[1][2 + 5].eq(F::neg(want[1][2 + 4])) && !want[0][2 + 4].is_zero(), "decompress: x = x0 or -x0 as the sign says");
            if (c.what == "mixed") check(want[0][4].eq(u(11)) && want[0][5].eq(u(2)) && want[0][6].eq(F::one()) && want[0][7].eq(F::one()) && want[0][1].eq(u(14)) && want[1][6].is_zero() && want[1][7].is_zero(), "mixed: sqrt(121) = 11, 23 = 2 * 11 + 1 and 22 = 2 * 11");
            {   // the plain marker on the root columns: refused, with the words it always had -- as a prefix under the any-order builder
                std::vector<uint32_t> plain_cols = c.unknown;
                plain_cols.insert(plain_cols.end(), c.roots.begin(), c.roots.end());
                const std::vector<uint8_t> plain = pattern(s, plain_cols, {}, c.quotients);
                const Plan t = in_order(s, plain), t_any = any_order(s, plain);
                const std::string text = "row " + std::to_string(c.first_root_row) + ": unknown column " + std::to_string(c.first_root_col) + " occurs in A and in B";
                check(t.error == ERR_TWO_MATRICES && t.error_row == c.first_root_row && t.error_col == c.first_root_col && t.message == text,
                      c.what + ": with the plain marker the matrix order is refused at the first square-root row, in the words it had");
                check(t_any.error == ERR_TWO_MATRICES && t_any.error_row == c.first_root_row && t_any.message.compare(0, text.size(), text) == 0 &&
                          t_any.message.compare(text.size(), 27, "; in any row order: column ") == 0,
                      c.what + ": ... and in any order: the same refusal as a prefix, then the column that stays unknown");
            }
            const uint32_t nr = (uint32_t)s.nr();
            for (int variant = 0; variant < 4; ++variant) {
                std::vector<uint32_t> order(nr);
                for (uint32_t i = 0; i < nr; ++i) order[i] = variant == 0 ? nr - 1 - i : i;
                if (variant > 0)
                    for (uint32_t i = nr; i > 1; --i) std::swap(order[i - 1], order[next_u64() % i]);
                keep_groups(order, c.groups);
                System t = s.permuted(order);
                const std::string tag = c.what + (variant ? ", permutation " + std::to_string(variant) : std::string(", reversed"));
                for (uint32_t wide : {WIDE_STEPS, 2u}) {
                    const Plan q = any_order(t, unknown, wide);
                    check(q.error == OK && q.message.empty() && q.steps.size() == p.steps.size() && q.pairs.size() == p.pairs.size() && q.divs.size() == p.divs.size() &&
                              count_kind(q, KIND_SQRT) == c.roots.size(),
                          tag + ": plans");
                    if (q.error != OK) continue;
                    check(q.reordered, tag + ": a reordered plan");
                    check(well_sorted(q), tag + ": sorted by (level, kind, row), launches in step");
                    check(column_levels(t, q) == levels, tag + ": every column keeps its level");
                    for (int round = 0; round < c.rounds; ++round) {
                        std::vector<Fr> z = c.given(round);
                        bool ok = execute(t, q, z) == NONE && z.size() == want[round].size();
                        for (size_t j = 0; ok && j < z.size(); ++j) ok = z[j].eq(want[round][j]);
                        check(ok, tag + ": executes to the in-order assignment");
                    }
                }
            }
        }
    }

    // ---- 6. a square-root row that waits for its C side, which a LATER row computes.  0 one | 1 a, 2 b given | 3 v, 4 u
    //   row 0: u * u = v      row 1: (a + b) * 1 = v
    void waiting_root() {
        const Fr one = F::one();
        System s; s.mw = 4;
        s.add(Row{{one, 4}}, Row{{one, 4}}, Row{{one, 3}});
        s.add(Row{{one, 1}, {one, 2}}, Row{{one, 0}}, Row{{one, 3}});
        const std::vector<uint8_t> unknown = pattern(s, {3}, {4});
        const Plan first = in_order(s, unknown), p = any_order(s, unknown);
        check(first.error == ERR_MANY_UNKNOWNS && first.error_row == 0, "waiting root: in matrix order the row has two unknowns and is refused");
        bool ok = p.error == OK && p.reordered && p.steps.size() == 2 && p.steps[0].kind == KIND_C && p.steps[0].row == 1 && p.steps[0].level == 1;
        if (ok) {
            Step want{0, 0, 4, KIND_SQRT, 2};
            ok = same_step(p.steps[1], want) && p.launches.size() == 1 && same_launch(p.launches[0], Launch{0, 2, LAUNCH_CHAIN, 1}) && well_sorted(p);
        }
        check(ok, "waiting root: it waits for its C side and is then taken as a square-root row, one level up");
        if (!ok) return;
        std::vector<Fr> z = {one, u(40), u(9), marker(), sqrt_marker()};
        check(execute(s, p, z) == NONE && z[3].eq(u(49)) && z[4].eq(u(7)) && rows_hold(s, z), "waiting root: 40 + 9 = 49 = 7^2");
        // reversed decompression in small: the row  u * k = x  has the opener's shape and is examined first; the square-root row releases it
        //   0 one | 1 x | 2 c, 3 k given | 4 u          row 0: u * k = x      row 1: u * u = c
        System d; d.m0 = 2; d.mw = 3;
        d.add(Row{{one, 4}}, Row{{one, 3}}, Row{{one, 1}});
        d.add(Row{{one, 4}}, Row{{one, 4}}, Row{{one, 2}});
        const Plan q = any_order(d, pattern(d, {1}, {4}));
        check(q.error == OK && q.reordered && q.steps.size() == 2 && q.pairs.empty() && q.steps[0].kind == KIND_SQRT && q.steps[0].row == 1 && q.steps[0].level == 1 &&
                  q.steps[1].kind == KIND_C && q.steps[1].row == 0 && q.steps[1].level == 2,
              "released: a square-root row releases an opener registered over its root");
        std::vector<Fr> w = {one, marker(), u(36), F::neg(one), sqrt_marker()};
        check(q.error == OK && execute(d, q, w) == NONE && w[4].eq(u(6)) && w[1].eq(F::neg(u(6))) && rows_hold(d, w), "released: ... and executes");
    }

    // ---- 7. a non-residue is stuck at its own row, its neighbours untouched; under a reordered plan it is the root cause
    void stuck() {
        const Fr one = F::one(), g = u(C::ID == 0 ? 7 : 5);
        {   // 0 one | 1, 3, 5 c_i given | 2, 4, 6 u_i
            System s; s.mw = 6;
            for (uint32_t i = 0; i < 3; ++i) s.add(Row{{one, 2 + 2 * i}}, Row{{one, 2 + 2 * i}}, Row{{one, 1 + 2 * i}});
            for (uint32_t wide : {WIDE_STEPS, 1u}) {
                const Plan p = in_order(s, pattern(s, {}, {2, 4, 6}), wide);
                std::vector<Fr> z = {one, u(9), sqrt_marker(), g, sqrt_marker(), u(16), sqrt_marker()};
                std::vector<uint32_t> rows;
                check(p.error == OK && execute(s, p, z, &rows) == 1 && rows == std::vector<uint32_t>({1}) && z[2].eq(u(3)) && z[4].is_zero() && z[6].eq(u(4)),
                      "stuck: the non-residue is stuck at row 1 with zero stored; rows 0 and 2 complete");
            }
        }
        {   // 0 one | 1 c given | 2 u, 3 w          row 0: w * u = 1 (reads the stored zero and sticks too, at a SMALLER row)      row 1: u * u = c
            System s; s.mw = 3;
            s.add(Row{{one, 3}}, Row{{one, 2}}, Row{{one, 0}});
            s.add(Row{{one, 2}}, Row{{one, 2}}, Row{{one, 1}});
            const Plan p = any_order(s, pattern(s, {3}, {2}));
            std::vector<Fr> z = {one, g, sqrt_marker(), marker()}, fine = {one, u(4), sqrt_marker(), marker()};
            std::vector<uint32_t> rows;
            check(p.error == OK && p.reordered && execute(s, p, z, &rows) == ((uint64_t)1 << 32 | 1) && rows == std::vector<uint32_t>({1, 0}) && z[2].is_zero() && z[3].is_zero(),
                  "stuck: under a reordered plan the word is (level 1, row 1): the square-root row, not the inversion of the stored zero at row 0");
            check(p.error == OK && execute(s, p, fine) == NONE && fine[2].eq(u(2)) && F::mul(fine[3], u(2)).eq(one), "stuck: ... and a residue completes");
        }
    }

    int run() {
        shapes();
        marker_elsewhere();
        markers();
        roots();
        corpus();
        waiting_root();
        stuck();
        return report();
    }
};

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381");
    Suite<pm::BnCurve> bn("bn254");
    return (bls.run() | bn.run()) ? 1 : 0;
}
