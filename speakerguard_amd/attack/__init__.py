from .SirenAttack import SirenAttack  # noqa: F401
